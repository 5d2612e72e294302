"""What ``LoopClosing::CorrectLoop`` reads and writes of ``Map`` / ``KeyFrame``
/ ``MapPoint``, as index arrays.

A keyframe is an index into the lists given at construction and grown by
``add_keyframe``, a map point an index into ``mps``. The slot tables (``KeyFrame::mvpMapPoints``) and the
observation maps (``MapPoint::mObservations``) are separate state, as in the
reference: ``AddObservation`` overwrites, and nothing here assumes that the two
agree or that a point sits in one slot per keyframe. Pointer-ordered containers
are walked in keyframe-index order (docs/ORACLE_ASSUMPTIONS.md A26).
"""
from __future__ import annotations

import numpy as np

from ._lib import GFError
from .matcher import MAP_POINT_DTYPE
from .orb import KEYPOINT_DTYPE


class LoopMap:
    def __init__(self, info, kf_kps, kf_desc, kf_mp, mps, mp_desc, mp_bad=None, observations=None, kf_bad=None,
                 distinctive=None, kf_Tcw=None, ref_kf=None, kf_id=None, first_kf=None, found=None, visible=None):
        """info: the FrameInfo every keyframe shares; kf_kps / kf_desc / kf_mp:
        per keyframe its undistorted keypoints, [n, 32] descriptors and slot
        table (map point id per keypoint, -1 = NULL); mps (MAP_POINT_DTYPE),
        mp_desc [M, 32], mp_bad [M]: the map points; observations: per point a
        dict keyframe -> slot (default: read off the slot tables, the later
        slot winning as AddObservation does); kf_bad: KeyFrame::isBad();
        distinctive(desc, offsets, current) -> (best, rows): the
        ComputeDistinctiveDescriptors used (default: the device's); kf_Tcw
        [nkf, 4, 4]: the poses (default identity); ref_kf [M]: mpRefKF per point
        (default its first observing keyframe, -1 without one); kf_id: mnId
        per keyframe, strictly increasing (default the index); first_kf /
        found / visible [M]: mnFirstKFid, mnFound, mnVisible per point
        (defaults: the reference keyframe's mnId, 1 and 1, as the constructor
        at MapPoint.cc:31-34 sets them)."""
        self.info = info
        self.kf_kps = [np.ascontiguousarray(k, KEYPOINT_DTYPE) for k in kf_kps]
        self.kf_desc = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in kf_desc]
        self.slots = [np.ascontiguousarray(s, np.int32).copy() for s in kf_mp]
        self.nkf = len(self.kf_kps)
        self.kf_bad = np.zeros(self.nkf, bool) if kf_bad is None else np.asarray(kf_bad).astype(bool).copy()
        self.mps = np.ascontiguousarray(mps, MAP_POINT_DTYPE).copy()
        self.mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32).copy()
        n = len(self.mps)
        self.mp_bad = np.zeros(n, bool) if mp_bad is None else np.asarray(mp_bad).astype(bool).copy()
        # bumped whenever a point's descriptor row really changes: what a search made earlier must be redone for
        self.desc_epoch = np.zeros(n, np.int64)
        if observations is None:
            self.obs = [dict() for _ in range(n)]
            for k, s in enumerate(self.slots):
                for idx in np.nonzero(s >= 0)[0]:
                    self.obs[int(s[idx])][k] = int(idx)
        else:
            self.obs = [dict(o) for o in observations]
        self._distinctive = distinctive
        self.Tcw = (np.tile(np.eye(4, dtype=np.float32), (self.nkf, 1, 1)) if kf_Tcw is None
                    else np.ascontiguousarray(kf_Tcw, np.float32).reshape(self.nkf, 4, 4).copy())
        self.kf_id = np.arange(self.nkf, dtype=np.int32) if kf_id is None else np.asarray(kf_id, np.int32).copy()
        self.ref_kf = (np.asarray([min(o) if o else -1 for o in self.obs], np.int32).reshape(-1) if ref_kf is None
                       else np.asarray(ref_kf, np.int32).copy())
        self.first_kf = (np.where(self.ref_kf >= 0, self.kf_id[np.maximum(self.ref_kf, 0)], -1).astype(np.int64)
                         if first_kf is None else np.asarray(first_kf, np.int64).copy())
        self.found = np.ones(n, np.int32) if found is None else np.asarray(found, np.int32).copy()
        self.visible = np.ones(n, np.int32) if visible is None else np.asarray(visible, np.int32).copy()
        self.corrected_by = np.full(n, -1, np.int32)   # mnCorrectedByKF (a keyframe index)
        self.corrected_ref = np.full(n, -1, np.int32)  # mnCorrectedReference
        # mnFuseTargetForKF per keyframe / mnFuseCandidateForKF per point: the mnId of the keyframe whose
        # SearchInNeighbors stamped it last, -1 = never stamped (docs/ORACLE_ASSUMPTIONS.md A28)
        self.fuse_target_for = np.full(self.nkf, -1, np.int64)
        self.fuse_candidate_for = np.full(n, -1, np.int64)
        # the covisibility graph: mConnectedKeyFrameWeights, the ordered covisibles with their weights,
        # mpParent / mbFirstConnection and the loop edges
        self.weights = [dict() for _ in range(self.nkf)]
        self.ordered = [[] for _ in range(self.nkf)]
        self.ordered_w = [[] for _ in range(self.nkf)]
        self.parent = [-1] * self.nkf
        self.first_connection = [True] * self.nkf
        self.loop_edges = [[] for _ in range(self.nkf)]
        # mbNotErase / mbToBeErased (KeyFrame.cc:474-508)
        self.not_erase = np.zeros(self.nkf, bool)
        self.to_be_erased = np.zeros(self.nkf, bool)
        # mBowVec as (words, values) / mFeatVec as a FeatureVector, None until ComputeBoW ran
        self.kf_bow = [None] * self.nkf
        self.kf_fv = [None] * self.nkf
        # the resident flat tables (maptables.ResidentTables), None = not attached: every method below that
        # writes obs, slots or mp_bad logs what it wrote there
        self.tables = None

    def attach_tables(self, ctx=None, applier=None, **policy):
        """Keep the flat tables of ``localmapping.culling_tables`` resident and
        up to date by journal (``maptables.ResidentTables``; ``applier`` and
        the capacity ``policy`` as there): the stages that read them then flush
        the journal instead of rebuilding them. -> the tables."""
        from .maptables import ResidentTables

        self.tables = ResidentTables(self, ctx, applier, **policy)
        return self.tables

    # ------------------------------------------------------------ Map
    def add_keyframe(self, kps, desc, slots, Tcw, kf_id=None) -> int:
        """``new KeyFrame(frame, pMap, pKFDB)`` + ``Map::AddKeyFrame``
        (KeyFrame.cc:30-54, Map.cc:33-39): a keyframe with the keypoints,
        descriptors, slot table (what tracking matched) and pose given, not
        bad, without connections, parent or BoW vectors, first connection
        pending. kf_id: its mnId, default the last one + 1; it must stay
        strictly increasing. No observation is added: the observation maps do
        not know the keyframe until ProcessNewKeyFrame, as in the reference.
        Returns its index."""
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1).copy()
        if not len(kps) == len(desc) == len(slots):
            raise GFError(-1, "keypoints, descriptors and slots: one row per keypoint")
        if len(slots) and (slots.min() < -1 or slots.max() >= len(self.mps)):
            raise GFError(-1, "a slot names a point outside the map")
        last = int(self.kf_id[-1]) if self.nkf else -1
        kf_id = last + 1 if kf_id is None else int(kf_id)
        if kf_id <= last:
            raise GFError(-1, f"mnId {kf_id} does not follow {last}")
        k = self.nkf
        self.kf_kps.append(kps)
        self.kf_desc.append(desc)
        self.slots.append(slots)
        self.kf_bad = np.append(self.kf_bad, False)
        self.Tcw = np.concatenate([self.Tcw.reshape(-1, 4, 4), np.asarray(Tcw, np.float32).reshape(1, 4, 4)])
        self.kf_id = np.append(self.kf_id, np.int32(kf_id))
        self.fuse_target_for = np.append(self.fuse_target_for, np.int64(-1))
        self.weights.append({})
        self.ordered.append([])
        self.ordered_w.append([])
        self.parent.append(-1)
        self.first_connection.append(True)
        self.loop_edges.append([])
        self.not_erase = np.append(self.not_erase, False)
        self.to_be_erased = np.append(self.to_be_erased, False)
        self.kf_bow.append(None)
        self.kf_fv.append(None)
        self.nkf = k + 1
        if self.tables is not None: self.tables.log_add_keyframe(k)
        return k

    # ------------------------------------------------------------ MapPoint
    def is_in_keyframe(self, p: int, kf: int) -> bool:
        """MapPoint::IsInKeyFrame: by the observation map."""
        return kf in self.obs[p]

    def add_observation(self, p: int, kf: int, idx: int) -> None:
        """MapPoint::AddObservation (MapPoint.cc:77-81): overwrites."""
        self.obs[p][int(kf)] = int(idx)
        if self.tables is not None: self.tables.log_obs_set(p, kf, idx)

    def new_map_point(self, pos, ref_kf: int) -> int:
        """``new MapPoint(pos, pRefKF, pMap)`` + ``Map::AddMapPoint``
        (MapPoint.cc:31-51): a point without observations, normal 0, min / max
        distance 0, mnFirstKFid = the reference keyframe's mnId, mnFound =
        mnVisible = 1, an all-zero descriptor. Returns its id."""
        p = len(self.mps)
        row = np.zeros(1, MAP_POINT_DTYPE)
        row["pos"] = np.asarray(pos, np.float32).reshape(3)
        self.mps = np.concatenate([self.mps, row])
        self.mp_desc = np.concatenate([self.mp_desc, np.zeros((1, 32), np.uint8)])
        self.mp_bad = np.append(self.mp_bad, False)
        self.desc_epoch = np.append(self.desc_epoch, np.int64(0))
        self.obs.append({})
        self.ref_kf = np.append(self.ref_kf, np.int32(ref_kf))
        self.first_kf = np.append(self.first_kf, np.int64(self.kf_id[int(ref_kf)]))
        self.found = np.append(self.found, np.int32(1))
        self.visible = np.append(self.visible, np.int32(1))
        self.corrected_by = np.append(self.corrected_by, np.int32(-1))
        self.corrected_ref = np.append(self.corrected_ref, np.int32(-1))
        self.fuse_candidate_for = np.append(self.fuse_candidate_for, np.int64(-1))
        if self.tables is not None: self.tables.log_new_map_point(p)
        return p

    def set_bad_point(self, p: int) -> None:
        """MapPoint::SetBadFlag (MapPoint.cc:117-131): the point turns bad, its
        observations are cleared and every observing keyframe erases the slot
        the observation named (EraseMapPointMatch(idx))."""
        p = int(p)
        obs, self.obs[p] = self.obs[p], {}
        self.mp_bad[p] = True
        for kf in sorted(obs):
            self.slots[kf][obs[kf]] = -1
        if self.tables is not None: self.tables.log_set_bad(p, obs)

    def erase_observation(self, p: int, kf: int) -> bool:
        """MapPoint::EraseObservation (MapPoint.cc:83-103): nothing when ``kf``
        does not observe the point; otherwise the entry goes, a reference
        keyframe equal to ``kf`` becomes the lowest remaining keyframe (``begin()``
        of the observation map; with no observation left ``ref_kf`` stays as it
        is, docs/ORACLE_ASSUMPTIONS.md A30), and a point left with two
        observations or fewer turns bad. -> whether it turned bad."""
        p, kf = int(p), int(kf)
        if kf not in self.obs[p]:
            return False
        del self.obs[p][kf]
        if self.tables is not None: self.tables.log_obs_erase(p, kf)
        if self.ref_kf[p] == kf and self.obs[p]:
            self.ref_kf[p] = min(self.obs[p])
        if len(self.obs[p]) <= 2:
            self.set_bad_point(p)
            return True
        return False

    def get_found_ratio(self, p: int) -> np.float32:
        """MapPoint::GetFoundRatio: ``static_cast<float>(mnFound)/mnVisible``."""
        return np.float32(self.found[p]) / np.float32(self.visible[p])

    def replace(self, a: int, b: int) -> None:
        """``a->Replace(b)`` (MapPoint.cc:136-170): a turns bad, its
        observations move to b (or are erased from a keyframe that b already
        observes), and b's descriptor is recomputed."""
        a, b = int(a), int(b)
        if a == b:
            return
        obs, self.obs[a] = self.obs[a], {}
        self.mp_bad[a] = True
        for kf in sorted(obs):
            idx = obs[kf]
            if not self.is_in_keyframe(b, kf):
                self.slots[kf][idx] = b  # ReplaceMapPointMatch
                self.add_observation(b, kf, idx)
            else:
                self.slots[kf][idx] = -1  # EraseMapPointMatch
        if self.tables is not None: self.tables.log_replace(a, obs)
        self.compute_distinctive_descriptors([b])

    def compute_distinctive_descriptors(self, ids) -> None:
        """MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:197-262) of the
        given points over ``gf_distinctive_descriptors``: the observations of
        non-bad keyframes in observation-map order; a bad or observation-less
        point is left as it is."""
        ids = [int(p) for p in ids if not self.mp_bad[int(p)] and self.obs[int(p)]]
        if not ids:
            return
        rows, offs = [], [0]
        for p in ids:
            for kf in sorted(self.obs[p]):
                if not self.kf_bad[kf]:
                    rows.append(self.kf_desc[kf][self.obs[p][kf]])
            offs.append(len(rows))
        if not rows:
            return
        fn = self._distinctive
        if fn is None:
            from .matcher import compute_distinctive_descriptors as fn
        cur = self.mp_desc[ids]
        _, out = fn(np.asarray(rows, np.uint8).reshape(-1, 32), np.asarray(offs, np.int32), cur)
        changed = np.any(out != cur, axis=1)
        for p, row, ch in zip(ids, out, changed):
            if ch:
                self.mp_desc[p] = row
                self.desc_epoch[p] += 1

    def update_normal_and_depth(self, ids) -> None:
        """MapPoint::UpdateNormalAndDepth (MapPoint.cc:285-324) of the given
        points on the host. ``cv::norm`` is a double sum, cast to float; a
        ``Mat / scalar`` is one float factor ``(float)(1 / scalar)``
        (docs/ORACLE_ASSUMPTIONS.md A22); the rest is float in the reference's
        order. A bad point returns as in the reference; one without
        observations or reference keyframe, where the reference divides by
        zero, is left as it is."""
        from .matcher import camera_center

        f32 = np.float32
        sf, scales = f32(self.info.scale_factor), self.info.scale_factors()
        nlev = len(scales)
        centre = {}

        def norm(d):
            return f32(np.sqrt((np.float64(d[0]) * np.float64(d[0]) + np.float64(d[1]) * np.float64(d[1]))
                               + np.float64(d[2]) * np.float64(d[2])))

        for p in ids:
            p = int(p)
            ref = int(self.ref_kf[p])
            if self.mp_bad[p] or not self.obs[p] or ref < 0 or not len(self.kf_kps[ref]):
                continue
            pos = self.mps["pos"][p].astype(f32)
            normal = np.zeros(3, f32)
            for kf in sorted(self.obs[p]):
                if kf not in centre:
                    centre[kf] = camera_center(self.Tcw[kf])
                d = pos - centre[kf]
                normal = normal + d * f32(1.0 / np.float64(norm(d)))
            if ref not in centre:
                centre[ref] = camera_center(self.Tcw[ref])
            dist = norm(pos - centre[ref])
            level = int(self.kf_kps[ref]["octave"][self.obs[p].get(ref, 0)])  # observations[pRefKF]: 0 when absent
            self.mps["min_dist"][p] = ((f32(1.0) / sf) * dist) / scales[level]
            self.mps["max_dist"][p] = (sf * dist) * scales[nlev - 1 - level]
            self.mps["normal"][p] = normal * f32(1.0 / len(self.obs[p]))

    def update_normal_and_depth_batch(self, ids, ctx=None) -> None:
        """:meth:`update_normal_and_depth` of the given points in one
        ``gf_update_normal_and_depth`` call: the observation rows in
        observation-map order as CSR, the camera centre of every keyframe, and
        per point the reference keyframe and the octave of
        ``observations[pRefKF]`` in it (slot 0 when the reference keyframe does
        not observe the point, as ``map::operator[]`` gives). A point is
        independent of every other, so the result is that of the per-point
        method, bit for bit."""
        from .matcher import camera_center, update_normal_and_depth

        ids = [int(p) for p in ids]
        if not ids:
            return
        offs, rows = [0], []
        ref_kf, ref_level = np.full(len(ids), -1, np.int32), np.zeros(len(ids), np.int32)
        for j, p in enumerate(ids):
            ref = int(self.ref_kf[p])
            if not (self.mp_bad[p] or not self.obs[p] or ref < 0 or not len(self.kf_kps[ref])):
                rows.extend(sorted(self.obs[p]))
                ref_kf[j] = ref
                ref_level[j] = int(self.kf_kps[ref]["octave"][self.obs[p].get(ref, 0)])
            offs.append(len(rows))
        if not rows:
            return
        Ow = np.stack([camera_center(T) for T in self.Tcw]) if self.nkf else np.zeros((0, 3), np.float32)
        nr, mn, mx = update_normal_and_depth(self.info, self.mps["pos"][ids], offs, rows, Ow, ref_kf, ref_level,
                                             self.mps["normal"][ids], self.mps["min_dist"][ids],
                                             self.mps["max_dist"][ids], ctx)
        self.mps["normal"][ids] = nr
        self.mps["min_dist"][ids] = mn
        self.mps["max_dist"][ids] = mx

    # ------------------------------------------------------------ KeyFrame
    def set_pose(self, kf: int, Tcw) -> None:
        """KeyFrame::SetPose."""
        self.Tcw[kf] = np.asarray(Tcw, np.float32).reshape(4, 4)

    def add_loop_edge(self, kf: int, other: int) -> None:
        """KeyFrame::AddLoopEdge (KeyFrame.cc:461-466): a set; the keyframe is
        not to be erased from now on."""
        self.not_erase[kf] = True
        if other not in self.loop_edges[kf]:
            self.loop_edges[kf].append(int(other))

    def set_not_erase(self, kf: int) -> None:
        """KeyFrame::SetNotErase (KeyFrame.cc:474-478)."""
        self.not_erase[int(kf)] = True

    def set_erase(self, kf: int, db=None):
        """KeyFrame::SetErase (KeyFrame.cc:480-494): the protection ends unless
        the keyframe has loop edges, and a SetBadFlag that was deferred
        meanwhile runs now. -> the log of :meth:`set_bad_keyframe`, or None
        when none was pending."""
        kf = int(kf)
        if not self.loop_edges[kf]:
            self.not_erase[kf] = False
        if self.to_be_erased[kf]:
            return self.set_bad_keyframe(kf, db)
        return None

    def erase_map_point_match(self, kf: int, idx: int) -> None:
        """KeyFrame::EraseMapPointMatch(idx)."""
        self.slots[int(kf)][int(idx)] = -1
        if self.tables is not None: self.tables.log_slot(kf, idx, -1)

    def erase_connection(self, kf: int, other: int) -> None:
        """KeyFrame::EraseConnection (KeyFrame.cc:596-610)."""
        if other in self.weights[kf]:
            del self.weights[kf][other]
            self.update_best_covisibles(kf)

    def children(self, kf: int) -> set:
        """KeyFrame::GetChilds of a keyframe that is not bad, derived from the
        parents: ``{c : parent[c] == kf and not kf_bad[c]}``. mspChildrens
        needs no state of its own here: a child enters it through
        ChangeParent / the first UpdateConnections, which also set
        ``parent[c]``; ChangeParent is called only from SetBadFlag, which moves
        every child of the keyframe that turns bad to another parent; and
        EraseChild is called only by a keyframe that turns bad, on its parent.
        So the set of a keyframe that is not bad is those whose parent it is,
        less the ones that turned bad."""
        kf = int(kf)
        return {c for c in range(self.nkf) if self.parent[c] == kf and not self.kf_bad[c]}

    def set_bad_keyframe(self, kf: int, db=None) -> dict:
        """KeyFrame::SetBadFlag (KeyFrame.cc:497-588). The first keyframe
        (mnId 0) returns; a ``not_erase`` keyframe only sets ``to_be_erased``.
        Otherwise, in the reference's order: EraseConnection(kf) on every key
        of the weight map (those only: a keyframe that lists ``kf`` without
        being listed back keeps its entry); EraseObservation(kf) on every
        non-NULL slot in slot order; the weights and the ordered lists are
        cleared; the spanning tree is mended (:524-579: the children in index
        order, each child's ordered covisibles in list order, the parent
        candidates in index order and compared by mnId, ``w > max`` strict so
        the first maximum wins; the children without a link go to the original
        parent); the keyframe turns bad; ``db.erase(kf)`` when a keyframe
        database is given (its slot is the keyframe index).

        -> log dict: ``erased`` (False: returned or deferred), ``deferred``,
        ``observations``: the (point, keyframe, slot) entries EraseObservation
        removed, ``points_bad``: the points that turned bad, ``cleared``: the
        (keyframe, slot) entries their SetBadFlag erased, ``reparented``:
        (child, new parent) pairs, all in order."""
        kf = int(kf)
        log = dict(erased=False, deferred=False, observations=[], points_bad=[], cleared=[], reparented=[])
        if self.kf_id[kf] == 0:
            return log
        if self.not_erase[kf]:
            self.to_be_erased[kf] = True
            log["deferred"] = True
            return log
        for other in sorted(self.weights[kf]):
            self.erase_connection(other, kf)
        for p in self.slots[kf]:
            p = int(p)
            if p < 0 or kf not in self.obs[p]:
                continue
            log["observations"].append((p, kf, self.obs[p][kf]))
            rest = [(k, i) for k, i in sorted(self.obs[p].items()) if k != kf]
            if self.erase_observation(p, kf):
                log["points_bad"].append(p)
                log["cleared"].extend(rest)
        self.weights[kf], self.ordered[kf], self.ordered_w[kf] = {}, [], []
        parent = self.parent[kf]
        candidates = {parent} if parent >= 0 else set()
        children = sorted(self.children(kf))
        while children:
            best, pc, pp = -1, None, None
            for c in children:
                for v in self.ordered[c]:
                    for s in sorted(candidates):
                        if self.kf_id[v] == self.kf_id[s]:
                            w = self.weights[c].get(v, 0)  # GetWeight
                            if w > best:
                                best, pc, pp = w, c, int(v)
            if pc is None:
                break
            self.parent[pc] = pp  # ChangeParent
            log["reparented"].append((pc, pp))
            candidates.add(pc)
            children.remove(pc)
        for c in children:
            self.parent[c] = parent
            log["reparented"].append((c, parent))
        self.kf_bad[kf] = True
        if db is not None:
            db.erase(kf)
        log["erased"] = True
        return log

    def to_essgraph_map(self) -> dict:
        """The map dict ``optimizer.EssGraphArrays`` takes."""
        return dict(kf_id=self.kf_id.copy(), Tcw=self.Tcw.copy(), parent=list(self.parent),
                    cov=[(list(o), list(w)) for o, w in zip(self.ordered, self.ordered_w)],
                    loop_edges=[sorted(e) for e in self.loop_edges], pos=self.mps["pos"].copy(),
                    bad=self.mp_bad.copy(), ref=self.ref_kf.copy(), corrected_ref=self.corrected_ref.copy())

    def add_map_point(self, kf: int, p: int, idx: int) -> None:
        """KeyFrame::AddMapPoint."""
        self.slots[kf][idx] = p
        if self.tables is not None: self.tables.log_slot(kf, idx, p)

    def get_map_points(self, kf: int) -> set:
        """KeyFrame::GetMapPoints (KeyFrame.cc:238-251): the non-bad points of
        the slot table."""
        s = self.slots[kf]
        s = s[s >= 0]
        return set(int(p) for p in s[~self.mp_bad[s]])

    def update_best_covisibles(self, kf: int) -> None:
        """KeyFrame::UpdateBestCovisibles (KeyFrame.cc:141-160): the ordered
        list rebuilt from every weight, heaviest first, the higher index first
        among equals (the sort of (weight, KeyFrame*) pairs, reversed)."""
        pairs = sorted((w, k) for k, w in self.weights[kf].items())[::-1]
        self.ordered[kf] = [k for _, k in pairs]
        self.ordered_w[kf] = [w for w, _ in pairs]

    def add_connection(self, kf: int, other: int, weight: int) -> None:
        """KeyFrame::AddConnection (KeyFrame.cc:126-139)."""
        if self.weights[kf].get(other) == weight:
            return
        self.weights[kf][other] = weight
        self.update_best_covisibles(kf)

    def update_connections(self, kf: int) -> None:
        """KeyFrame::UpdateConnections (KeyFrame.cc:332-421). The weight map
        receives every counted keyframe; the ordered list those with 15 shared
        points or more, or the single heaviest one; the others hear of it
        through AddConnection."""
        kf = int(kf)
        counter = {}
        for p in self.slots[kf]:
            if p < 0 or self.mp_bad[p]:
                continue
            for k in self.obs[int(p)]:
                if k != kf:
                    counter[k] = counter.get(k, 0) + 1
        if not counter:
            return
        nmax, kmax, pairs = 0, None, []
        for k in sorted(counter):
            if counter[k] > nmax:
                nmax, kmax = counter[k], k
            if counter[k] >= 15:
                pairs.append((counter[k], k))
                self.add_connection(k, kf, counter[k])
        if not pairs:
            pairs.append((nmax, kmax))
            self.add_connection(kmax, kf, nmax)
        pairs = sorted(pairs)[::-1]
        self.weights[kf] = dict(counter)
        self.ordered[kf] = [k for _, k in pairs]
        self.ordered_w[kf] = [w for w, _ in pairs]
        if self.first_connection[kf] and kf != 0:
            self.parent[kf] = self.ordered[kf][0]
            self.first_connection[kf] = False

    def connections_counts(self, kfs, ctx=None, counter=None):
        """The counting and ordering of UpdateConnections (KeyFrame.cc:332-403)
        for every keyframe of ``kfs`` in one ``gf_update_connections_dev``
        launch over the flat tables of the map as it stands
        (``localmapping.culling_tables``). It reads slot tables, observation
        maps and bad flags only, none of which UpdateConnections writes, so any
        number of keyframes can be counted before the first is applied.
        counter: a callable with the signature of
        ``localmapping.update_connections_counts`` used instead of the device
        (the CPU tests inject the restatement's).
        -> (weights [len(kfs), nkf] int32, 0 = not in the counter; per keyframe
        ``(ordered keyframes, their weights)`` as lists)."""
        from .localmapping import _CovisTables

        return _CovisTables(self, ctx, counter).count(kfs)

    def apply_connections(self, kf: int, weights_row, ordered_kf, ordered_w) -> None:
        """The rest of UpdateConnections (KeyFrame.cc:365-418) from one row of
        :meth:`connections_counts`: nothing when the counter is empty (:365);
        otherwise AddConnection(kf, w) on every listed keyframe (:386, :393),
        the keyframe's weight map (every counted keyframe), ordered list and
        ordered weights (:409-411), and on its first connection the head of
        the list as parent (:413-418). The first-connection test is that of
        :meth:`update_connections`, so that the two stay equal field by field:
        the map's first keyframe never gets a parent. Keyframe ids increase
        with the index, so mnId 0 (the reference's test) can sit nowhere else;
        the two tests differ only on a map whose first keyframe has another id
        (docs/ORACLE_ASSUMPTIONS.md A26). The listed keyframes are distinct, so
        the order of the AddConnection calls (here list order, there index
        order) changes nothing."""
        kf = int(kf)
        ordered_kf, ordered_w = [int(k) for k in ordered_kf], [int(w) for w in ordered_w]
        if not ordered_kf:
            return
        for k, w in zip(ordered_kf, ordered_w):
            self.add_connection(k, kf, w)
        row = np.asarray(weights_row)
        self.weights[kf] = {int(k): int(row[k]) for k in np.nonzero(row > 0)[0]}
        self.ordered[kf], self.ordered_w[kf] = ordered_kf, ordered_w
        if self.first_connection[kf] and kf != 0:
            self.parent[kf] = ordered_kf[0]
            self.first_connection[kf] = False

    def update_connections_batch(self, kfs, ctx=None, counter=None) -> None:
        """:meth:`update_connections` of every keyframe of ``kfs``, in that
        order: one :meth:`connections_counts` for all of them, then
        :meth:`apply_connections` one by one. Equal to the serial calls because
        no apply writes what a count reads."""
        kfs = [int(k) for k in kfs]
        weights, ordered = self.connections_counts(kfs, ctx, counter)
        for i, kf in enumerate(kfs):
            self.apply_connections(kf, weights[i], *ordered[i])

    def get_connected_keyframes(self, kf: int) -> set:
        """KeyFrame::GetConnectedKeyFrames: every key of the weight map."""
        return set(self.weights[kf])

    def observation_rows(self) -> np.ndarray:
        """Every observation as a (point, keyframe, slot) row, point-major,
        keyframe-index order."""
        out = [(p, kf, o[kf]) for p, o in enumerate(self.obs) for kf in sorted(o)]
        return np.asarray(out, np.int32).reshape(-1, 3)
