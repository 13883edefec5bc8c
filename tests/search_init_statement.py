"""The checker of oracle_search_for_initialization and orbx_search_for_initialization_device: an independent statement of
ORBmatcher::SearchForInitialization (reference src/ORBmatcher.cc:706-821) with Frame::GetFeaturesInArea (src/Frame.cc:655-724) and
ComputeThreeMaxima (:2303-2344), in plain Python / numpy, one frame-1 keypoint at a time.  It shares no code with oracle/orb_oracle.cpp: there is
no cell traversal (the candidates are a box test over the keypoints that are in the grid, sorted by grid position; the cell window of the reference
only cuts that list, and `box_outside_cells` counts what it cuts), the Hamming distance is a sum over unpacked bits, the histogram is sorted instead
of scanned, and every binary32 step is a numpy float32 scalar operation.

search_init_walk(...) is the walk; exit codes, one per frame-1 keypoint, in the reference's order:
  LEVEL              octave > 0                                                                          (:722-723)
  NO_CAND            vIndices2.empty(): one of the four early returns of GetFeaturesInArea (`early` says which) or an empty box   (:727-728)
  ALL_HIDDEN         every candidate skipped by vMatchedDistance[i2] <= dist                              (:744-745)
  TH_LOW             best distance > 50                                                                   (:759)
  RATIO              best >= second * mfNNratio                                                           (:761)
  ACCEPTED           matched a free keypoint of frame 2
  ACCEPTED_STEALING  matched a keypoint that another request held                                         (:763-767)
A request that was accepted keeps its code when it is stolen from or dropped by the histogram later: the counters `stolen` and `hist_dropped` tell.

synchronous_rounds(...) is the claim in the header of extractorb_amd/csrc/k_match.hip, written down apart from the kernel: all requests decide at
once from the previous round's decisions, a keypoint of frame 2 hides itself at the smallest distance among the EARLIER requests that currently
hold it, and the rounds repeat until nothing changes.  tests/test_search_init_edges.py asserts that this fixed point is the walk."""
import numpy as np

f32 = np.float32
EXITS = ("LEVEL", "NO_CAND", "ALL_HIDDEN", "TH_LOW", "RATIO", "ACCEPTED", "ACCEPTED_STEALING")
LEVEL, NO_CAND, ALL_HIDDEN, TH_LOW_EXIT, RATIO, ACCEPTED, ACCEPTED_STEALING = range(len(EXITS))
TH_LOW, HISTO_LENGTH = 50, 30      # ORBmatcher.cc:37-38
BIG = 1 << 30
COLS, ROWS = 64, 48


def grid_tables(n2, idx2):
    """(inside2, grid_pos2) of a frame whose mGrid holds the keypoints idx2 in traversal order"""
    inside = np.zeros(n2, bool); pos = np.zeros(n2, int)
    inside[idx2] = True; pos[idx2] = np.arange(len(idx2))
    return inside, pos


def cell_window(x, y, r, bounds):
    """GetFeaturesInArea's cell window in binary32 (Frame.cc:666-688): (early return 1..4 or 0, (minCX, maxCX, minCY, maxCY))"""
    if bounds is None:
        return 0, None
    min_x, max_x, min_y, max_y = (f32(v) for v in bounds)
    w_inv, h_inv = f32(f32(COLS) / f32(max_x - min_x)), f32(f32(ROWS) / f32(max_y - min_y))
    r = f32(r)
    c0 = max(0, int(np.floor(f32(f32(f32(x - min_x) - r) * w_inv))))
    if c0 >= COLS: return 1, None
    c1 = min(COLS - 1, int(np.ceil(f32(f32(f32(x - min_x) + r) * w_inv))))
    if c1 < 0: return 2, None
    r0 = max(0, int(np.floor(f32(f32(f32(y - min_y) - r) * h_inv))))
    if r0 >= ROWS: return 3, None
    r1 = min(ROWS - 1, int(np.ceil(f32(f32(f32(y - min_y) + r) * h_inv))))
    if r1 < 0: return 4, None
    return 0, (c0, c1, r0, r1)


def _candidate_lists(k1, k2, inside2, grid_pos2, prev, window, bounds):
    """per frame-1 keypoint: None (level > 0) or (early, candidates in traversal order, number the cell window cut from the box)"""
    n2 = len(k2)
    order = sorted((i for i in range(n2) if inside2[i] and k2["octave"][i] == 0), key=lambda i: grid_pos2[i])
    x2, y2 = k2["x"].astype(np.float32), k2["y"].astype(np.float32)
    cell = None
    if bounds is not None and n2:
        min_x, max_x, min_y, max_y = (f32(v) for v in bounds)
        w_inv, h_inv = f32(f32(COLS) / f32(max_x - min_x)), f32(f32(ROWS) / f32(max_y - min_y))
        half_away = lambda v: np.copysign(np.floor(np.abs(v.astype(np.float64)) + 0.5), v).astype(np.int64)      # std::round (PosInGrid, Frame.cc:728-729)
        cell = (half_away(((x2 - min_x).astype(np.float32) * w_inv).astype(np.float32)), half_away(((y2 - min_y).astype(np.float32) * h_inv).astype(np.float32)))
    w = f32(window)
    order = np.array(order, np.int64)
    ox, oy = x2[order], y2[order]
    out = []
    for i1 in range(len(k1)):
        if k1["octave"][i1] > 0:
            out.append(None); continue
        x, y = f32(prev[i1][0]), f32(prev[i1][1])
        early, win = cell_window(x, y, w, bounds)
        cand, cut = [], 0
        if not early and len(order):
            box = (np.abs(ox - x) < w) & (np.abs(oy - y) < w)      # Frame.cc:717, binary32 differences
            if win is not None:
                inside = (win[0] <= cell[0][order]) & (cell[0][order] <= win[1]) & (win[2] <= cell[1][order]) & (cell[1][order] <= win[3])
                cut = int((box & ~inside).sum()); box &= inside
            cand = order[box].tolist()
        out.append((early, cand, cut))
    return out


def _distances(d1, d2):
    """[N1, N2] Hamming distances"""
    if len(d1) == 0 or len(d2) == 0:
        return np.zeros((len(d1), len(d2)), np.int64)
    b1 = np.unpackbits(np.asarray(d1, np.uint8).reshape(-1, 32), axis=1).astype(np.int16)
    b2 = np.unpackbits(np.asarray(d2, np.uint8).reshape(-1, 32), axis=1).astype(np.int16)
    return (b1 @ (1 - b2).T + (1 - b1) @ b2.T).astype(np.int64)


def _choose(cand, dist_row, hidden_at, nnratio):
    """one request's scan (:739-769) against the hidden distances `hidden_at(i2)`: (exit code, slot or -1, distance)"""
    best, best2, bi, seen = BIG, BIG, -1, False
    for i2 in cand:
        dist = int(dist_row[i2])
        if hidden_at(i2) <= dist:
            continue
        seen = True
        if dist < best:
            best2, best, bi = best, dist, i2
        elif dist < best2:
            best2 = dist
    if not seen:
        return ALL_HIDDEN, -1, BIG
    if best > TH_LOW:
        return TH_LOW_EXIT, -1, BIG
    if not f32(best) < f32(f32(best2 if best2 < BIG else 2 ** 31) * f32(nnratio)):      # (float)INT_MAX = 2^31
        return RATIO, -1, BIG
    return ACCEPTED, bi, best


def rotation_bin(a1, a2):
    rot = f32(f32(a1) - f32(a2))                                   # :775-779
    if rot < 0:
        rot = f32(rot + f32(360))
    b = int(np.floor(float(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH)))) + 0.5))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes):
    """ComputeThreeMaxima: the kept bins.  Strict > in the scan: of equal bins the lowest indices win."""
    order = sorted(range(len(sizes)), key=lambda i: (-sizes[i], i))
    top = [order[0] if sizes[order[0]] > 0 else -1]
    mx = sizes[order[0]]
    for o in order[1:3]:
        top.append(o if sizes[o] > 0 and not f32(sizes[o]) < f32(f32(0.1) * f32(mx)) else -1)
    if top[1] == -1:
        top[2] = -1
    return top


def search_init_walk(k1, d1, k2, d2, inside2, grid_pos2, prev, window, nnratio, check, bounds=None):
    """Returns dict(nmatches, m12 [N1] list, prev [N1, 2] float32, exit [N1], early [N1] (which early return of GetFeaturesInArea, 0 = none),
    bin [N1] (rotHist bin of an acceptance, -1 = none), hist [30] sizes, kept_bins, and the counters stolen, hist_dropped, second_choice,
    max_first_round_holders, first_round_holders {holders: slots}, box_outside_cells).  bounds = None: no cell window at all (pure box test)."""
    n1 = len(k1)
    cands = _candidate_lists(k1, k2, inside2, grid_pos2, prev, window, bounds)
    dist = _distances(d1, d2)
    m12 = [-1] * n1; m21 = {}; mdist = {}
    code = np.zeros(n1, np.int32); early = np.zeros(n1, np.int32); rbin = np.full(n1, -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    first = {}                                                    # against empty tables: request -> slot
    nm = stolen = second_choice = cut = 0
    for i1 in range(n1):
        if cands[i1] is None:
            code[i1] = LEVEL; continue
        early[i1], cand, c = cands[i1]
        cut += c
        if not cand:
            code[i1] = NO_CAND; continue
        e0, s0, _ = _choose(cand, dist[i1], lambda i2: BIG, nnratio)
        if e0 == ACCEPTED:
            first[i1] = s0
        code[i1], bi, best = _choose(cand, dist[i1], lambda i2: mdist.get(i2, BIG), nnratio)
        if code[i1] != ACCEPTED:
            continue
        if bi in m21:
            m12[m21[bi]] = -1; nm -= 1; stolen += 1; code[i1] = ACCEPTED_STEALING
        m12[i1] = bi; m21[bi] = i1; mdist[bi] = best; nm += 1
        second_choice += first.get(i1, -1) != bi
        if check:
            rbin[i1] = rotation_bin(k1["angle"][i1], k2["angle"][bi])
            hist[rbin[i1]].append(i1)
    sizes = [len(h) for h in hist]
    top, dropped = [], 0
    if check:
        top = three_maxima(sizes)
        for b in range(HISTO_LENGTH):
            if b in top:
                continue
            for i1 in hist[b]:
                if m12[i1] >= 0:
                    m12[i1] = -1; nm -= 1; dropped += 1
    prev = np.array(prev, np.float32).reshape(n1, 2).copy()
    for i1 in range(n1):
        if m12[i1] >= 0:
            prev[i1] = (k2["x"][m12[i1]], k2["y"][m12[i1]])       # :815-817
    per_slot = {}
    for s in first.values():
        per_slot[s] = per_slot.get(s, 0) + 1
    holders = {}
    for c in per_slot.values():
        holders[c] = holders.get(c, 0) + 1
    return dict(nmatches=nm, m12=m12, prev=prev, exit=code, early=early, bin=rbin, hist=sizes, kept_bins=top, stolen=stolen, hist_dropped=dropped,
                second_choice=second_choice, max_first_round_holders=max(per_slot.values(), default=0), first_round_holders=holders,
                box_outside_cells=cut)


def brute_force_search(k1, d1, k2, d2, inside2, grid_pos2, prev, window, nnratio, check):
    """the walk's outputs alone (nmatches, vnMatches12, vbPrevMatched), candidates by the box test only"""
    res = search_init_walk(k1, d1, k2, d2, inside2, grid_pos2, prev, window, nnratio, check)
    return res["nmatches"], res["m12"], res["prev"]


def counts(res):
    """exit name -> number of frame-1 keypoints"""
    return {name: int((res["exit"] == c).sum()) for c, name in enumerate(EXITS)}


def synchronous_rounds(k1, d1, k2, d2, inside2, grid_pos2, prev, window, nnratio, bounds=None, max_rounds=None):
    """The parallel fixed point.  Returns (decisions: per frame-1 keypoint (slot, distance) or None, rounds): `rounds` counts every round that was
    computed, the last one (which changed nothing) included."""
    n1 = len(k1)
    cands = _candidate_lists(k1, k2, inside2, grid_pos2, prev, window, bounds)
    dist = _distances(d1, d2)
    requests = [i1 for i1 in range(n1) if cands[i1] is not None]
    dec = {i1: None for i1 in requests}
    rounds = 0
    while max_rounds is None or rounds < max_rounds:
        rounds += 1
        held = {}                                                 # slot -> [(request, distance)] of the previous round
        for i1 in requests:
            if dec[i1] is not None:
                held.setdefault(dec[i1][0], []).append((i1, dec[i1][1]))
        new = {}
        for i1 in requests:
            hidden_at = lambda i2: min((d for r, d in held.get(i2, ()) if r < i1), default=BIG)
            e, s, best = _choose(cands[i1][1], dist[i1], hidden_at, nnratio) if cands[i1][1] else (NO_CAND, -1, BIG)
            new[i1] = (s, best) if e == ACCEPTED else None
        changed = new != dec
        dec = new
        if not changed:
            break
    return [dec.get(i1) for i1 in range(n1)], rounds


def tables_of_decisions(decisions):
    """vnMatches12 before the histogram from the final decisions: a slot belongs to its LAST holder (every earlier one was stolen from)"""
    owner = {}
    for i1, d in enumerate(decisions):
        if d is not None:
            owner[d[0]] = i1
    return [d[0] if d is not None and owner[d[0]] == i1 else -1 for i1, d in enumerate(decisions)]
