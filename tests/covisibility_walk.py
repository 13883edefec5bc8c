"""The independent statement of orbx_covisibility_device and orbx_keyframe_redundancy_device: KeyFrame::UpdateConnections (reference
src/KeyFrame.cc:388-511), the voting half of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:3030-3102) and the test inside
LocalMapping::KeyFrameCulling's loop (src/LocalMapping.cc:977-1043), written with the reference's own structures: KeyFrame and MapPoint
objects, mObservations as a std::map keyed by the KeyFrame's address (StdMap below: a dict that iterates in key order), KFcounter as
another, vPairs as a list of (weight, address) pairs sorted ascending and reversed by push_front, the early return, numpy float32 for the
one product.  Nothing here knows ranks, counters indexed by anything, or lanes.

What the ENTRY adds to the reference is stated apart (checked / duplicate_keys): the indices a subject reads are checked before anything
of it is written, and two frames with one key are refused for the whole call.

MUTANTS are one-line changes of the walk; tests/test_covisibility.py names the scene that notices each, or says why none can."""
import numpy as np

f32 = np.float32
UPDATE_CONNECTIONS, LOCAL_KEYFRAMES = 0, 1
STATUS = ("OK", "EMPTY", "TRUNCATED", "BAD_INDEX", "DUPLICATE_KEY")
OK, EMPTY, TRUNCATED, BAD_INDEX, DUPLICATE_KEY = range(5)
REDUNDANCY_STATUS = ("OK", "SKIPPED", "BAD_INDEX")
RD_OK, RD_SKIPPED, RD_BAD_INDEX = range(3)
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_counter", "<i4"), ("n_ordered", "<i4"), ("nmax", "<i4"), ("kf_max", "<i4")])
REDUNDANCY_DTYPE = np.dtype([("status", "<i4"), ("n_mps", "<i4"), ("n_redundant", "<i4"), ("redundant", "<i4")])
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

MUTANTS = {
    "frame_order": "the maps iterate in device-frame order instead of address order",
    "ties_key_ascending": "equal weights of the ordered list in ascending key order",
    "th_gt": "a count enters the ordered list when it is > th",
    "nmax_ge": "pKFmax is the LAST keyframe that reaches the largest count (>= at :440 / :3094)",
    "no_self_test": "the subject votes for itself (mnId == mnId dropped at :415)",
    "map_test_in_frame_mode": "UpdateLocalKeyFrames skips observers of another map",
    "self_test_in_frame_mode": "UpdateLocalKeyFrames skips d_subject_kf",
    "bad_excluded_from_frame_count": "UpdateLocalKeyFrames does not count a bad observer at all",
    "bad_listed_in_frame_mode": "the isBad() skip of :3091 dropped",
    "bad_counted_in_update": "UpdateConnections counts a bad observer",
    "other_map_counted": "UpdateConnections counts an observer of another map",
    "bad_map_point_votes": "a bad MapPoint's observations are walked",
    "slots_once": "a MapPoint that stands in two slots votes once",
    "single_pair_dropped": "no count >= th leaves the ordered list empty",
    "list_length_for_observations": "Observations() is the length of the observation list",
    "observations_ge": "Observations() >= thObs",
    "octave_lt": "scaleLeveli < scaleLevel + 1",
    "octave_plus_two": "scaleLeveli <= scaleLevel + 2",
    "subject_counts_itself": "pKFi == pKF is not skipped",
    "slot_ge": "a slot is redundant when nObs >= thObs",
    "bad_observers_skipped_in_culling": "KeyFrameCulling tests its observers for isBad()",
    "final_ge": ">= at :1043",
    "product_double": "redundant_th * nMPs in double",
    "depth_ge": "depth >= mThDepth is skipped",
    "depth_le_zero": "depth <= 0 is skipped",
    "nan_depth_skipped": "a NaN depth is skipped (the test written as !(0 <= depth <= th))",
}


class StdMap(dict):
    """std::map: iteration in key order.  `order` says what a key's order is (the address; the frame under the frame_order mutant)"""

    def __init__(self, order):
        super().__init__()
        self.order = order

    def __iter__(self):
        return iter(sorted(dict.keys(self), key=self.order))

    def items(self):
        return [(k, self[k]) for k in self]


class KeyFrame:
    def __init__(self, frame, key, flags, map_id):
        self.frame, self.key, self.map = frame, int(key), map_id            # key: the KeyFrame* address
        self.bad, self.initial = bool(flags & 1), bool(flags & 2)

    def isBad(self):
        return self.bad


class MapPoint:
    def __init__(self, bad, observations, nobs):
        self.bad, self.make, self.nObs = bad, observations, nobs            # observations() -> {KeyFrame: row} in address order
        self.made = None

    @property
    def mObservations(self):                                                # (built when the walk first reads it: what it never reads may be junk)
        if self.made is None:
            self.made = self.make()
        return self.made

    def isBad(self):
        return self.bad

    def Observations(self):
        return self.nObs


# ---- what the entry checks before the reference's code runs -----------------------------------------------------------------------------------
def duplicate_keys(s):
    return len(set(int(k) for k in s["kf_key"])) != s["n_frames"]


def subject_slots(s, j):
    n = min(max(int(s["subject_n"][j]), 0), s["capacity"])
    return [int(m) for m in s["subject_mp"][j, :n]]


def list_ok(s, m):
    o0, o1, total = int(s["obs_off"][m]), int(s["obs_off"][m + 1]), int(s["obs_off"][s["n_points"]])
    return o0 >= 0 and o1 >= o0 and o1 <= total


def vote_checked(s, j):
    """every index subject j's vote reads lies inside its table"""
    if s["mode"] == UPDATE_CONNECTIONS and not -1 <= int(s["subject_kf"][j]) < s["n_frames"]:
        return False
    for m in subject_slots(s, j):
        if m == -1:
            continue
        if not 0 <= m < s["n_points"]:
            return False
        if s["mp_flags"][m] & 1:
            continue
        if not list_ok(s, m):
            return False
        if any(not 0 <= int(f) < s["n_frames"] for f in s["obs"][int(s["obs_off"][m]):int(s["obs_off"][m + 1]), 0]):
            return False
    return True


def redundancy_checked(s, j, kf, mutant=None):
    for i, m in enumerate(subject_slots(s, j)):
        if m == -1:
            continue
        if not 0 <= m < s["n_points"]:
            return False
        if s["mp_flags"][m] & 1 or far(s, kf, i, mutant):
            continue
        if not list_ok(s, m):
            return False
        nobs = int(s["mp_nobs"][m]) if s["mp_nobs"] is not None else int(s["obs_off"][m + 1]) - int(s["obs_off"][m])
        if nobs > s["th_obs"]:
            for f, row in s["obs"][int(s["obs_off"][m]):int(s["obs_off"][m + 1])]:
                if not 0 <= int(f) < s["n_frames"] or not 0 <= int(row) < min(max(int(s["n_out"][f]), 0), s["capacity"]):
                    return False
    return True


def far(s, kf, i, mutant=None):
    """:992-996, as written"""
    if s["monocular"]:
        return False
    d, th = s["depth"][kf, i], s["th_depth"][kf]
    if mutant == "nan_depth_skipped":
        return not (f32(0) <= d <= th)
    return bool((d >= th if mutant == "depth_ge" else d > th) or (d <= 0 if mutant == "depth_le_zero" else d < 0))


# ---- the reference's objects from the tables ------------------------------------------------------------------------------------------------
def build(s, mutant=None):
    order = (lambda kf: kf.frame) if mutant == "frame_order" else (lambda kf: kf.key)
    maps = s["kf_map"] if s.get("kf_map") is not None else np.zeros(s["n_frames"], np.int32)
    kfs = [KeyFrame(f, s["kf_key"][f] if "kf_key" in s else f, int(s["kf_flags"][f]), int(maps[f])) for f in range(s["n_frames"])]
    mps = {}

    def map_point(m):
        if m not in mps:
            o0, o1 = int(s["obs_off"][m]), int(s["obs_off"][m + 1])

            def observations():
                obs = StdMap(order)
                for f, row in s["obs"][o0:o1]:
                    obs[kfs[int(f)]] = int(row)
                return obs
            nobs = int(s["mp_nobs"][m]) if s.get("mp_nobs") is not None and mutant != "list_length_for_observations" else o1 - o0
            mps[m] = MapPoint(bool(s["mp_flags"][m] & 1), observations, nobs)
        return mps[m]
    return kfs, map_point, order


# ---- KeyFrame::UpdateConnections -------------------------------------------------------------------------------------------------------------
def update_connections(vpMP, this, mpMap, th, order, mutant=None):
    """returns None at the early return, else (mConnectedKeyFrameWeights as a list in map order, ordered keyframes, ordered weights, nmax,
    pKFmax)"""
    KFcounter = StdMap(order)
    seen = set()
    for pMP in vpMP:
        if pMP is None:
            continue
        if pMP.isBad() and mutant != "bad_map_point_votes":
            continue
        if mutant == "slots_once":
            if id(pMP) in seen:
                continue
            seen.add(id(pMP))
        for pKF, _ in pMP.mObservations.items():
            if (pKF is this and mutant != "no_self_test") or (pKF.isBad() and mutant != "bad_counted_in_update") or \
                    (pKF.map != mpMap and mutant != "other_map_counted"):
                continue
            KFcounter[pKF] = KFcounter.get(pKF, 0) + 1
    if not KFcounter:
        return None
    nmax, pKFmax = 0, None
    vPairs = []
    for pKF, n in KFcounter.items():
        if n >= nmax if mutant == "nmax_ge" else n > nmax:
            nmax, pKFmax = n, pKF
        if n > th if mutant == "th_gt" else n >= th:
            vPairs.append((n, pKF))
    if not vPairs and mutant != "single_pair_dropped":
        vPairs.append((nmax, pKFmax))
    vPairs.sort(key=lambda pr: (pr[0], -order(pr[1]) if mutant == "ties_key_ascending" else order(pr[1])))      # pair<int,KeyFrame*>::operator<
    lKFs, lWs = [], []
    for n, pKF in vPairs:
        lKFs.insert(0, pKF)                                      # push_front
        lWs.insert(0, n)
    return KFcounter.items(), lKFs, lWs, nmax, pKFmax


# ---- Tracking::UpdateLocalKeyFrames, :3030-3102 ------------------------------------------------------------------------------------------------
def update_local_keyframes(vpMP, order, mutant=None, this=None, mpMap=None):
    keyframeCounter = StdMap(order)
    for pMP in vpMP:
        if pMP is not None and (not pMP.isBad() or mutant == "bad_map_point_votes"):
            for pKF, _ in pMP.mObservations.items():
                if mutant == "map_test_in_frame_mode" and pKF.map != mpMap:
                    continue
                if mutant == "self_test_in_frame_mode" and pKF is this:
                    continue
                if mutant == "bad_excluded_from_frame_count" and pKF.isBad():
                    continue
                keyframeCounter[pKF] = keyframeCounter.get(pKF, 0) + 1
    mx, pKFmax = 0, None
    mvpLocalKeyFrames = []
    for pKF, n in keyframeCounter.items():
        if pKF.isBad() and mutant != "bad_listed_in_frame_mode":
            continue
        if n >= mx if mutant == "nmax_ge" else n > mx:
            mx, pKFmax = n, pKF
        mvpLocalKeyFrames.append((pKF, n))
    return mvpLocalKeyFrames, mx, pKFmax


def poisoned_vote_outputs(s):
    ns, cc = s["n_subjects"], s["conn_capacity"]
    blocks = {k: np.full((ns, cc), POISON, np.int32) for k in ("counter_kf", "counter_w", "ordered_kf", "ordered_w")}
    return dict(blocks, result=np.frombuffer(bytes([0xEE]) * (RESULT_DTYPE.itemsize * ns), RESULT_DTYPE).copy())


POISON = np.int32(-286331154)                            # 0xEEEEEEEE


def walk_vote(s, mutant=None):
    out = poisoned_vote_outputs(s)
    cc = s["conn_capacity"]
    res = out["result"]
    for j in range(s["n_subjects"]):
        res[j] = (OK, 0, 0, 0, -1)
    if duplicate_keys(s):
        res["status"] = DUPLICATE_KEY
        return out
    kfs, map_point, order = build(s, mutant)
    update = s["mode"] == UPDATE_CONNECTIONS
    for j in range(s["n_subjects"]):
        if not vote_checked(s, j):
            res[j]["status"] = BAD_INDEX
            continue
        vpMP = [None if m == -1 else map_point(m) for m in subject_slots(s, j)]
        sub_kf = int(s["subject_kf"][j]) if s.get("subject_kf") is not None else -1
        this = kfs[sub_kf] if 0 <= sub_kf < s["n_frames"] else None
        mpMap = int(s["subject_map"][j]) if s.get("subject_map") is not None else 0
        if update:
            got = update_connections(vpMP, this, mpMap, s["th"], order, mutant)
            if got is None:
                res[j]["status"] = EMPTY
                continue
            counter, lKFs, lWs, nmax, pKFmax = got
            for i, (pKF, w) in enumerate(zip(lKFs[:cc], lWs[:cc])):
                out["ordered_kf"][j, i], out["ordered_w"][j, i] = pKF.frame, w
        else:
            counter, nmax, pKFmax = update_local_keyframes(vpMP, order, mutant, this, mpMap)
            lKFs = []
        for i, (pKF, w) in enumerate(counter[:cc]):
            out["counter_kf"][j, i], out["counter_w"][j, i] = pKF.frame, w
        res[j] = (TRUNCATED if len(counter) > cc or len(lKFs) > cc else OK, len(counter), len(lKFs), nmax, -1 if pKFmax is None else pKFmax.frame)
    return out


# ---- LocalMapping::KeyFrameCulling, the body of its loop for one pKF (:977-1043) ---------------------------------------------------------------
def keyframe_redundant(s, pKF, vpMapPoints, kfs, mutant=None):
    """returns None for the `continue` of :977, else (nMPs, nRedundantObservations, the test of :1043, the slots' states)"""
    if pKF.initial or pKF.isBad():
        return None
    thObs = s["th_obs"]
    nRedundantObservations = nMPs = 0
    states = []
    for i, pMP in enumerate(vpMapPoints):
        states.append(0)
        if pMP is None or pMP.isBad():
            continue
        if far(s, pKF.frame, i, mutant):
            continue
        nMPs += 1
        states[i] = 1
        if pMP.Observations() >= thObs if mutant == "observations_ge" else pMP.Observations() > thObs:
            scaleLevel = int(s["kps_un"][pKF.frame, i]["octave"])
            nObs = 0
            for pKFi, leftIndex in pMP.mObservations.items():
                if pKFi is pKF and mutant != "subject_counts_itself":
                    continue
                if mutant == "bad_observers_skipped_in_culling" and pKFi.isBad():
                    continue
                scaleLeveli = int(s["kps_un"][pKFi.frame, leftIndex]["octave"])
                limit = scaleLevel + (2 if mutant == "octave_plus_two" else 1)
                if scaleLeveli < limit if mutant == "octave_lt" else scaleLeveli <= limit:
                    nObs += 1                                    # (the break at nObs > thObs changes nothing)
            if nObs >= thObs if mutant == "slot_ge" else nObs > thObs:
                nRedundantObservations += 1
                states[i] = 2
    if mutant == "product_double":
        product = float(s["redundant_th"]) * nMPs
    else:
        product = f32(s["redundant_th"]) * f32(nMPs)              # int * float: the int converts to float, ONE float product
        assert product.dtype == f32
    lhs = nRedundantObservations if mutant == "product_double" else f32(nRedundantObservations)
    return nMPs, nRedundantObservations, bool(lhs >= product if mutant == "final_ge" else lhs > product), states


def poisoned_redundancy_outputs(s):
    ns = s["n_subjects"]
    return dict(result=np.frombuffer(bytes([0xEE]) * (REDUNDANCY_DTYPE.itemsize * ns), REDUNDANCY_DTYPE).copy(),
                slot_state=np.full((ns, s["capacity"]), 0xEE, np.uint8))


def walk_redundancy(s, mutant=None):
    out = poisoned_redundancy_outputs(s)
    res = out["result"]
    kfs, map_point, _ = build(s, mutant)
    for j in range(s["n_subjects"]):
        res[j] = (RD_OK, 0, 0, 0)
        kf = int(s["subject_kf"][j])
        if not 0 <= kf < s["n_frames"]:
            res[j]["status"] = RD_BAD_INDEX
            continue
        if s["kf_flags"][kf] & 3:                                # the reference tests :977 before it reads anything of the keyframe
            res[j]["status"] = RD_SKIPPED
            continue
        if not redundancy_checked(s, j, kf, mutant):
            res[j]["status"] = RD_BAD_INDEX
            continue
        vpMapPoints = [None if m == -1 else map_point(m) for m in subject_slots(s, j)]
        nMPs, nRed, redundant, states = keyframe_redundant(s, kfs[kf], vpMapPoints, kfs, mutant)
        res[j] = (RD_OK, nMPs, nRed, int(redundant))
        out["slot_state"][j, :len(states)] = states
    return out


def walk_scene(s, mutant=None):
    return walk_vote(s, mutant) if s["kind"] == "vote" else walk_redundancy(s, mutant)
