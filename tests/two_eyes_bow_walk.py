"""The checker of orbx_search_by_bow_two_eyes_device: a fresh statement of ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches)
(reference src/ORBmatcher.cc:269-471) for two-camera frames (F.Nleft != -1: the else branch :340-367 and :373-433) as a sequential walk
over Python lists, in the reference's CONCATENATED index space: keypoint i of the left eye is i, keypoint j of the right eye Nleft + j, for
the keyframe (the index space of pKF->GetMapPointMatches()) and for the frame (vpMapPointMatches) alike.

A FeatureVector is (nodes, idx): std::map<NodeId, vector<unsigned>> flattened in (node, list) order.  merge_feature_vectors builds the
concatenated one from the two eyes' own (what ComputeBoW gives per descriptor block)."""
import numpy as np

HISTO_LENGTH = 30
POPCOUNT = np.array([bin(b).count("1") for b in range(256)], np.int32)


def merge_feature_vectors(fv_left, fv_right, n_left):
    """mFeatVec of descriptors stacked left over right from the eyes' own FeatureVectors: FeatureVector::addFeature appends in feature
    order and every left index precedes every right one, so a node's list is the left eye's list followed by the right eye's (+ n_left)."""
    nodes = np.concatenate([np.asarray(fv_left[0], np.uint32), np.asarray(fv_right[0], np.uint32)])
    idx = np.concatenate([np.asarray(fv_left[1], np.int64), np.asarray(fv_right[1], np.int64) + n_left])
    order = np.argsort(nodes, kind="stable")      # stable: left entries stay in front of right ones, each in its own order
    return nodes[order], idx[order].astype(np.uint32)


def _as_map(fv):
    out = {}
    for node, i in zip(np.asarray(fv[0]).tolist(), np.asarray(fv[1]).tolist()):
        out.setdefault(node, []).append(i)
    return sorted(out.items())


def three_maxima(counts):
    """ORBmatcher::ComputeThreeMaxima (:2303-2344) on the bins' sizes"""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(counts):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, i
        elif s > m3:
            m3, i3 = s, i
    if np.float32(m2) < np.float32(0.1) * np.float32(m1):
        i2 = i3 = -1
    elif np.float32(m3) < np.float32(0.1) * np.float32(m1):
        i3 = -1
    return i1, i2, i3


def search_by_bow_two_eyes(kf_fv, f_fv, kf_flags, kf_angle, kf_desc, f_angle, f_desc, n_left, nnratio=0.7, th_low=50, check_orientation=True):
    """kf_fv / f_fv: concatenated FeatureVectors; kf_flags[i] bit 0: the keyframe's feature i holds a good MapPoint; *_angle, *_desc: the
    keypoint angles / descriptors, left eye's then right eye's; n_left = F.Nleft.  Returns dict(n = the return value, matches = for
    every feature of the frame the keyframe feature whose MapPoint it holds or -1, and the counters: left_writes, right_writes,
    right_without_left (right writes whose left ratio test failed), right_own_ratio_fail (right writes the disabled ratio test of :403 would
    have refused), stopped_by_left (keyframe features with a right best within th_low and no left best within it), removals (:452-468))."""
    f32 = np.float32
    kf_desc = np.asarray(kf_desc, np.uint8).reshape(-1, 32); f_desc = np.asarray(f_desc, np.uint8).reshape(-1, 32)
    NF = len(f_desc)
    held = [-1] * NF                                  # vpMapPointMatches, as the keyframe feature the MapPoint came from
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    factor = f32(1.0) / f32(HISTO_LENGTH)
    c = dict(left_writes=0, right_writes=0, right_without_left=0, right_own_ratio_fail=0, stopped_by_left=0, removals=0)
    nmatches = 0
    f_map = dict(_as_map(f_fv))

    def push(real_kf, idx_f):
        rot = f32(kf_angle[real_kf]) - f32(f_angle[idx_f])
        if rot < 0:
            rot = f32(rot + f32(360.0))
        b = int(np.floor(float(f32(rot * factor)) + 0.5))          # round(): half away from zero, rot >= 0
        if b == HISTO_LENGTH:
            b = 0
        assert 0 <= b < HISTO_LENGTH
        rot_hist[b].append(idx_f)

    for node, indices_kf in _as_map(kf_fv):           # the two maps walked in step meet exactly the common keys (:290-295, :434-443)
        indices_f = f_map.get(node)
        if indices_f is None:
            continue
        for real_kf in indices_kf:
            if not int(kf_flags[real_kf]) & 1:        # !pMP || pMP->isBad()
                continue
            d1, d2, best = 256, 256, -1
            d1r, d2r, best_r = 256, 256, -1
            open_f = [i for i in indices_f if held[i] < 0]
            if open_f:
                dist = POPCOUNT[f_desc[open_f] ^ kf_desc[real_kf]].sum(1).tolist()
                for i, d in zip(open_f, dist):
                    if i < n_left:
                        if d < d1:
                            d2, d1, best = d1, d, i
                        elif d < d2:
                            d2 = d
                    else:
                        if d < d1r:
                            d2r, d1r, best_r = d1r, d, i
                        elif d < d2r:
                            d2r = d
            if d1 <= th_low:
                left_ok = f32(d1) < f32(nnratio) * f32(d2)
                if left_ok:
                    if best < 0:
                        raise ValueError("the reference would write vpMapPointMatches[-1] (th_low >= 256)")
                    held[best] = real_kf
                    if check_orientation:
                        push(real_kf, best)
                    nmatches += 1
                    c["left_writes"] += 1
                if d1r <= th_low:                     # (its ratio test is `|| true`, :403)
                    if best_r < 0:
                        raise ValueError("the reference would write vpMapPointMatches[-1] (th_low >= 256)")
                    held[best_r] = real_kf
                    if check_orientation:
                        push(real_kf, best_r)
                    nmatches += 1
                    c["right_writes"] += 1
                    c["right_without_left"] += not left_ok
                    c["right_own_ratio_fail"] += not (f32(d1r) < f32(nnratio) * f32(d2r))
            elif d1r <= th_low:
                c["stopped_by_left"] += 1
    if check_orientation:
        keep = three_maxima([len(b) for b in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for idx_f in rot_hist[i]:
                held[idx_f] = -1
                nmatches -= 1
                c["removals"] += 1
    return dict(n=nmatches, matches=held, **c)
