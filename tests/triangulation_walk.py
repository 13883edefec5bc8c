"""The checker of orbx_search_for_triangulation_device: a fresh sequential statement of ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12,
vMatchedPairs, bOnlyStereo, bCoarse) (reference src/ORBmatcher.cc:965-1206) for one-camera keyframes (NLeft == -1, no mpCamera2: the
branches :994-1004 and :1099-1129 are not taken) with Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:122-144, from its line 130
on: F12 and the epipole are inputs), on Python lists with numpy binary32 scalars, in the reference's control flow: the running bestDist,
vbMatched2 created and tested and never set, rotHist as lists of keyframe-1 indices.

A FeatureVector is (nodes, idx): std::map<NodeId, vector<unsigned>> flattened in (node, list) order."""
import numpy as np

from two_eyes_bow_walk import HISTO_LENGTH, POPCOUNT, three_maxima

f32 = np.float32


def _as_map(fv):
    out = {}
    for node, i in zip(np.asarray(fv[0]).tolist(), np.asarray(fv[1]).tolist()):
        out.setdefault(node, []).append(i)
    return sorted(out.items())


def epipolar_constrain(x1, y1, x2, y2, F12, unc):
    """Pinhole.cpp:130-143: binary32 with every product, sum and the quotient rounded on its own; the last compare in double"""
    x1, y1, x2, y2 = f32(x1), f32(y1), f32(x2), f32(y2)
    a = f32(f32(f32(x1 * F12[0, 0]) + f32(y1 * F12[1, 0])) + F12[2, 0])
    b = f32(f32(f32(x1 * F12[0, 1]) + f32(y1 * F12[1, 1])) + F12[2, 1])
    c = f32(f32(f32(x1 * F12[0, 2]) + f32(y1 * F12[1, 2])) + F12[2, 2])
    num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
    den = f32(f32(a * a) + f32(b * b))
    if den == 0:
        return False
    with np.errstate(all="ignore"):
        dsqr = f32(f32(num * num) / den)
    return float(dsqr) < 3.84 * float(f32(unc))


def search_for_triangulation(fv1, fv2, mp1, mp2, kps1, kps2, u_right1, u_right2, desc1, desc2, F12, ep, scale_factors, level_sigma2,
                             only_stereo=False, coarse=False, th_low=50, check_orientation=True):
    """fv1 / fv2: FeatureVectors; mp1 / mp2[i] bit 0: GetMapPoint(i) != NULL; kps1 / kps2: mvKeysUn (x, y, angle, octave); u_right1 /
    u_right2: mvuRight, or None (no feature is stereo); desc1 / desc2 [N][32]; F12 [3][3] and ep [2] binary32; the extractor's
    mvScaleFactors / mvLevelSigma2.  Returns dict(n = the return value, matches12 = vMatches12, pairs = vMatchedPairs, and the counters:
    mp, stereo, disc, epi (candidates dropped for a MapPoint, by the stereo filter, by the epipole's disc, by the epipolar test), equal (best
    replaced by an EQUAL distance), shared (keyframe-2 features chosen by more than one keyframe-1 feature, counted per extra choice),
    removals (:1182-1191))."""
    desc1 = np.asarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    F12 = np.asarray(F12, np.float32).reshape(3, 3); ep = np.asarray(ep, np.float32).reshape(2)
    sf = np.asarray(scale_factors, np.float32); sig2 = np.asarray(level_sigma2, np.float32)
    N1, N2 = len(desc1), len(desc2)
    x1s, y1s, ang1 = kps1["x"], kps1["y"], kps1["angle"]
    x2s, y2s, ang2, oct2 = kps2["x"], kps2["y"], kps2["angle"], kps2["octave"]
    matched2 = [False] * N2                          # vbMatched2 (:1011): tested below, never set
    matches12 = [-1] * N1                            # vMatches12 (:1012)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    factor = f32(1.0) / f32(HISTO_LENGTH)
    c = dict(mp=0, stereo=0, disc=0, epi=0, equal=0, shared=0, removals=0)
    nmatches = 0
    map2 = dict(_as_map(fv2))
    for node, list1 in _as_map(fv1):                 # the two maps walked in step meet exactly the common keys (:1025-1172)
        list2 = map2.get(node)
        if list2 is None:
            continue
        d12 = POPCOUNT[desc1[list1][:, None, :] ^ desc2[list2][None, :, :]].sum(2).tolist()      # DescriptorDistance (:2349-2365)
        for a1, idx1 in enumerate(list1):
            if int(mp1[idx1]) & 1:                   # :1033-1039
                continue
            stereo1 = u_right1 is not None and u_right1[idx1] >= 0
            if only_stereo and not stereo1:          # :1043-1045
                continue
            best_dist, best_idx2 = th_low, -1        # :1057-1058
            for a2, idx2 in enumerate(list2):
                if matched2[idx2] or int(mp2[idx2]) & 1:          # :1067
                    c["mp"] += 1
                    continue
                stereo2 = u_right2 is not None and u_right2[idx2] >= 0
                if only_stereo and not stereo2:      # :1072-1074
                    c["stereo"] += 1
                    continue
                dist = d12[a1][a2]
                if dist > th_low or dist > best_dist:             # :1080
                    continue
                o = int(oct2[idx2])
                if not stereo1 and not stereo2:      # :1089-1097
                    ex = f32(ep[0] - f32(x2s[idx2])); ey = f32(ep[1] - f32(y2s[idx2]))
                    if f32(f32(ex * ex) + f32(ey * ey)) < f32(f32(100) * sf[o]):
                        c["disc"] += 1
                        continue
                if epipolar_constrain(x1s[idx1], y1s[idx1], x2s[idx2], y2s[idx2], F12, sig2[o]) or coarse:      # :1132
                    if best_idx2 >= 0 and dist == best_dist:
                        c["equal"] += 1
                    best_idx2, best_dist = idx2, dist
                else:
                    c["epi"] += 1
            if best_idx2 >= 0:                       # :1139-1158
                matches12[idx1] = best_idx2
                nmatches += 1
                if check_orientation:
                    rot = f32(f32(ang1[idx1]) - f32(ang2[best_idx2]))
                    if rot < 0:
                        rot = f32(rot + f32(360.0))
                    b = int(np.floor(float(f32(rot * factor)) + 0.5))          # round(): half away from zero, rot >= 0
                    if b == HISTO_LENGTH:
                        b = 0
                    assert 0 <= b < HISTO_LENGTH
                    rot_hist[b].append(idx1)
    if check_orientation:                            # :1174-1193
        keep = three_maxima([len(b) for b in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for idx1 in rot_hist[i]:
                matches12[idx1] = -1
                nmatches -= 1
                c["removals"] += 1
    pairs = [(i, m) for i, m in enumerate(matches12) if m >= 0]      # :1195-1203
    chosen = [m for _, m in pairs]
    c["shared"] = len(chosen) - len(set(chosen))
    return dict(n=nmatches, matches12=matches12, pairs=pairs, **c)
