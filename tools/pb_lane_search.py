#!/usr/bin/env python3
"""Deals the patch blur of k_describe<PB> over the 32 lanes of a keypoint so that every tile row's horizontal pass is computed once.

The ten column groups of the disc (rmax = 11, 15, 17, 18, 18, 18, 18, 16, 13, 6: k_describe_body.hpp) are laid end to end on two VIRTUAL
columns of 192 rows, one per DPP row of 16 lanes.  Lane l of a DPP row computes the horizontal sums of virtual rows 12 l .. 12 l + 11 (six row
pairs), receives the first three pairs of lane l + 1 (row_shl:1) and so holds virtual rows 12 l .. 12 l + 17, out of which it can blur the
twelve output rows 12 l .. 12 l + 11.  A group of n = 2 rmax + 1 output rows takes n + 6 virtual rows (its tile rows 18 - rmax .. 24 + rmax); the
last six outputs over them mix two groups and are not stored.  Constraints:
  * a group starts on an even virtual row (a lane then changes group between two row pairs: one address select per pair);
  * the stored outputs of a lane belong to ONE group (c_pbRun keeps one run per lane) and every lane stores at least one row;
  * a group lies inside one DPP row, its last stored row at most the row's virtual row 185 (lane 15 has no lower neighbour).
Among the layouts that fit, the one whose LDS instructions collide least in the 64 banks is printed as the two tables of the header
(cost = sum over the raw-tile loads and the blurred-tile stores of the largest number of lanes of the wave on one bank)."""
import itertools

RMAX = [11, 15, 17, 18, 18, 18, 18, 16, 13, 6]
N = [2 * r + 1 for r in RMAX]
LO = [18 - r for r in RMAX]
ROWS, LANES = 12, 16
PB_STRIDE_DW, BLUR_STRIDE_DW, RAW_DW, KP_DW = 11, 10, 476, 846      # kPbStride, kBlurStride, kPbRawBytes, kPbLds in dwords


def place(order):
    starts, ie, eprev = [], 0, None
    for g in order:
        s = ie + (ie & 1)
        if eprev is not None:
            s = max(s, ROWS * ((eprev - 1) // ROWS + 1))      # the next group's stored rows start in a later lane
        starts.append(s)
        eprev, ie = s + N[g], s + N[g] + 6
    return starts if ie <= ROWS * LANES else None


def lanes_of(order, starts):
    """per lane of one DPP row: (rowA, gA, rowB, gB, split, k0, g, o0, n) or None when the layout breaks a rule"""
    owner = [None] * (ROWS * LANES + 6)
    for g, s in zip(order, starts):
        for v in range(s, s + N[g] + 6):
            owner[v] = (g, LO[g] + v - s)
    out = []
    for l in range(LANES):
        v0 = ROWS * l
        own = owner[v0:v0 + ROWS]
        groups = [o[0] for o in own if o]
        if not groups:
            return None
        gA = groups[0]
        gB = groups[-1]
        ia = [i for i in range(ROWS) if own[i] and own[i][0] == gA]
        ib = [i for i in range(ROWS) if own[i] and own[i][0] == gB]
        rowA = own[ia[0]][1] - ia[0]
        rowB = own[ib[0]][1] - ib[0]
        if gA == gB:
            split = ROWS if ia[0] == 0 else 0        # (padding in front: the rows before a group are read as its B part)
            if split == 0 and rowB < 0:
                return None
            if split == ROWS and rowA + ROWS - 1 > 43:
                return None
        else:
            split = ib[0]                            # padding between the two is read as rows past A's end (row 43 at most: see the header)
            if rowA + split - 1 > 43:
                return None
        assert split % 2 == 0
        # stored outputs: virtual rows whose seven inputs belong to one group
        valid = []
        for k in range(ROWS):
            w = owner[v0 + k:v0 + k + 7]
            if all(w) and len({o[0] for o in w}) == 1 and w[0][1] <= 36 and abs(w[0][1] - 18) <= RMAX[w[0][0]]:
                valid.append((k, w[0][0], w[0][1]))
        if not valid or len({g for _, g, _ in valid}) != 1:
            return None
        k0, g, o0 = valid[0]
        n = len(valid)
        assert [k for k, _, _ in valid] == list(range(k0, k0 + n))
        if l == LANES - 1 and k0 + n > 6:
            return None
        out.append((rowA, gA, rowB, gB, split, k0, g, o0, n))
    return out


def cost(lanes32):
    c = 0
    for i in range(ROWS):
        for d in range(3):
            banks = {}
            for kp in range(2):
                for (rowA, gA, rowB, gB, split, *_rest) in lanes32:
                    a = ((rowA + i) * PB_STRIDE_DW + gA if i < split else (rowB + i) * PB_STRIDE_DW + gB) + d + kp * KP_DW
                    banks[a % 64] = banks.get(a % 64, set()) | {a}
            c += max(len(s) for s in banks.values())
    for k in range(ROWS):
        banks = {}
        for kp in range(2):
            for (*_r, k0, g, o0, n) in lanes32:
                if k0 <= k < k0 + n:
                    a = RAW_DW + (o0 + k - k0) * BLUR_STRIDE_DW + g + kp * KP_DW
                    banks[a % 64] = banks.get(a % 64, set()) | {a}
        c += max([len(s) for s in banks.values()] or [0])
    return c


def main():
    halves = {}
    for r in range(1, 10):
        for sub in itertools.combinations(range(10), r):
            if sum(N[g] + 6 for g in sub) > ROWS * LANES:
                continue
            best = []
            for order in itertools.permutations(sub):
                st = place(order)
                if st:
                    ln = lanes_of(order, st)
                    if ln:
                        best.append((order, st, ln))
            if best:
                halves[frozenset(sub)] = best
    found = []
    for sub, a_list in halves.items():
        rest = frozenset(range(10)) - sub
        if 9 not in sub or rest not in halves:
            continue
        for a in a_list:
            for b in halves[rest]:
                for first, second in ((a, b), (b, a)):
                    found.append((cost(first[2] + second[2]), first, second))
    found.sort(key=lambda t: t[0])
    print("layouts that fit:", len(found), " cost best / worst:", found[0][0], found[-1][0])
    c, a, b = found[0]
    print("DPP row 0: groups", a[0], "start at virtual rows", a[1])
    print("DPP row 1: groups", b[0], "start at virtual rows", b[1])
    lanes = a[2] + b[2]
    run = ["0x%06x" % (g | o0 << 8 | n << 16) for (*_r, g, o0, n) in lanes]
    src = []
    for (rowA, gA, rowB, gB, split, k0, *_r) in lanes:
        offA, offB = 44 * rowA + 4 * gA, 44 * rowB + 4 * gB + 1024
        assert 0 <= offA < 2048 and 0 <= offB < 4096
        src.append("0x%08x" % (offA | offB << 11 | split << 23 | k0 << 27))
    print("c_pbRun:", ", ".join(run))
    print("c_pbSrc:", ", ".join(src))
    print("horizontal passes:", 32 * ROWS, "issue slots; rows needed:", sum(n + 6 for n in N))


if __name__ == "__main__":
    main()
