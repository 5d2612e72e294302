"""Resident map tables: the flat tables of ``localmapping.culling_tables``
(plus the keypoint positions LocalBundleAdjustment reads) kept as state of a
:class:`~gf_orb_slam_amd.loopmap.LoopMap` and updated by a journal of the
map's own writes, instead of being rebuilt from the Python containers and
uploaded whole by every stage.

Layout ("slack CSR"). ``obs_off[p] .. obs_off[p + 1]`` is the capacity of row
``p``, not its length: inside it sit the live entries in ascending order of the
global keypoint index ``kf_off[kf] + idx`` (= ascending keyframe index, the
observation-map order), then -1 up to the capacity. The consuming kernels
(``kfcull.hip``, ``covis.hip``, ``lbagraph.hip``) bounds-test every entry and
skip -1, so they read such a table unchanged. Invariant: after every
:meth:`ResidentTables.flush`, the tables with the -1 entries dropped equal
``culling_tables(map)`` entry for entry.

Every write to ``LoopMap.obs``, ``LoopMap.slots[k][i]`` and ``LoopMap.mp_bad``
goes through a ``LoopMap`` method; with tables attached
(``LoopMap.attach_tables``) each of them logs what it wrote. Keyframes and
points are only ever appended, so the global keypoint index of an observation
never changes and new rows go at the tail. ``flush`` appends the new keyframes
and points, regrows the observation table when a touched row needs more than
its capacity (``gf_map_tables_move_dev``) and applies the journal in one
``gf_map_tables_apply_dev`` launch.
"""
from __future__ import annotations

import numpy as np

from ._lib import GFError, check, lib, ptr
from .orb import default_context

OBS_SET, OBS_ERASE, OBS_CLEAR = 0, 1, 2
MT_ROW = 1024  # GF_MT_ROW: the longest row k_tables_apply holds in LDS
MAX_KEYPOINTS = 4096
NAMES = ("kf_off", "octave", "slots", "kp_xy", "mp_bad", "obs_off", "obs_gkp")
_DTYPES = dict(kf_off=np.int32, octave=np.uint8, slots=np.int32, kp_xy=np.float32, mp_bad=np.uint8, obs_off=np.int32,
               obs_gkp=np.int32)


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def tables_apply(kf_off, slots, mp_bad, obs_off, obs_gkp, slot_g, slot_v, bad_p, row_ids, row_op_off, ops, ctx=None):
    """``gf_map_tables_apply`` on host arrays: the journal (slot writes
    ``slots[slot_g] = slot_v``, bad flags ``mp_bad[bad_p] = 1`` and, per touched
    row ``row_ids[r]``, the ops ``ops[row_op_off[r]:row_op_off[r + 1]]`` =
    (kind, kf, idx) in journal order) applied in place to ``slots`` (int32),
    ``mp_bad`` (uint8) and ``obs_gkp`` (int32), all contiguous. -> status [2]:
    rows left untouched for lack of room, ops skipped as out of range."""
    ctx = ctx or default_context()
    for a, dt in ((slots, np.int32), (mp_bad, np.uint8), (obs_gkp, np.int32)):
        if a.dtype != dt or not a.flags.c_contiguous:
            raise GFError(-1, "slots / mp_bad / obs_gkp: contiguous int32 / uint8 / int32, updated in place")
    kf_off, obs_off, slot_g, slot_v, bad_p, row_ids, row_op_off, ops = (
        _i32(a) for a in (kf_off, obs_off, slot_g, slot_v, bad_p, row_ids, row_op_off, ops))
    if not len(row_ids) and not len(row_op_off):
        row_op_off = np.zeros(1, np.int32)
    nkf, nmp = len(kf_off) - 1, len(mp_bad)
    if (nkf < 0 or len(obs_off) != nmp + 1 or len(slot_g) != len(slot_v) or len(ops) % 3
            or len(row_op_off) != len(row_ids) + 1 or kf_off[-1] != len(slots) or obs_off[-1] != len(obs_gkp)):
        raise GFError(-1, "table lengths disagree")
    status = np.zeros(2, np.int32)
    check(lib().gf_map_tables_apply(ctx.handle, nkf, ptr(kf_off), ptr(slots), nmp, ptr(mp_bad), ptr(obs_off),
                                    ptr(obs_gkp), len(slot_g), ptr(slot_g), ptr(slot_v), len(bad_p), ptr(bad_p),
                                    len(row_ids), ptr(row_ids), ptr(row_op_off), len(ops) // 3, ptr(ops), ptr(status)))
    return status


def tables_move(old_off, old_gkp, new_off, new_gkp, ctx=None):
    """``gf_map_tables_move`` on host arrays: every row's live entries copied,
    compacted and in order, to the row's start in ``new_gkp`` (contiguous
    int32, every entry written), -1 after them. -> status [1]: rows whose new
    capacity is below their live count (written as all -1)."""
    ctx = ctx or default_context()
    if new_gkp.dtype != np.int32 or not new_gkp.flags.c_contiguous:
        raise GFError(-1, "new_gkp: contiguous int32")
    old_off, old_gkp, new_off = _i32(old_off), _i32(old_gkp), _i32(new_off)
    nmp = max(len(old_off) - 1, 0)
    if len(new_off) != len(old_off) or (nmp and (old_off[-1] != len(old_gkp) or new_off[-1] != len(new_gkp))):
        raise GFError(-1, "table lengths disagree")
    status = np.zeros(1, np.int32)
    check(lib().gf_map_tables_move(ctx.handle, nmp, ptr(old_off), ptr(old_gkp), ptr(new_off), ptr(new_gkp),
                                   ptr(status)))
    return status


class _Buf:
    """A flat buffer with geometric spare capacity behind its used length: a
    numpy array on the host, a torch tensor on the device."""

    def __init__(self, owner, dtype):
        self.o, self.dtype, self.a, self.n = owner, dtype, None, 0

    def _alloc(self, cap):
        if self.o.host:
            return np.empty(cap, self.dtype)
        return self.o.torch.empty(cap, dtype=self.o.tdt[self.dtype], device=self.o.dev)

    def _put(self, lo, src):
        if not len(src):
            return
        src = np.ascontiguousarray(src, self.dtype).reshape(-1)
        if self.o.host:
            self.a[lo:lo + len(src)] = src
        else:
            self.a[lo:lo + len(src)].copy_(self.o.torch.from_numpy(src))

    def set(self, src):
        """The whole content replaced."""
        n = int(np.asarray(src).size)
        if self.a is None or len(self.a) < n:
            self.a = self._alloc(n + n // 4 + 16)
        self.n = n
        self._put(0, src)

    def reserve(self, n):
        """A fresh buffer of used length ``n``, content undefined."""
        self.a, self.n = self._alloc(n + n // 4 + 16), n

    def append(self, src):
        k = int(np.asarray(src).size)
        if self.a is None or self.n + k > len(self.a):
            old, n = self.a, self.n
            self.a = self._alloc((n + k) + (n + k) // 2 + 16)
            if old is not None and n:
                if self.o.host:
                    self.a[:n] = old[:n]
                else:
                    self.a[:n].copy_(old[:n])
        self._put(self.n, src)
        self.n += k

    def view(self):
        return self.a[:self.n]


class ResidentTables:
    """The resident table set of a LoopMap: ``kf_off``, ``octave``, ``slots``,
    ``kp_xy``, ``mp_bad``, ``obs_off`` and ``obs_gkp`` as device tensors with
    geometric spare capacity, host mirrors of ``kf_off``, ``obs_off`` and the
    per-row live count, and the journal of what the map wrote since the last
    :meth:`flush`. Built once from ``culling_tables(map)``.

    applier: a pair of callables with the signatures of :func:`tables_apply`
    and :func:`tables_move`, used instead of the device on host numpy copies of
    the tables (the CPU tests inject the restatement's).

    Capacity policy: a row is given ``max(min_cap, live + int(growth * live))``
    entries when the table is built or regrown; a new point's row ``min_cap``.
    """

    def __init__(self, map, ctx=None, applier=None, min_cap=8, growth=0.5):
        self.map, self.applier, self.host = map, applier, applier is not None
        self.min_cap, self.growth = int(min_cap), float(growth)
        if self.min_cap < 0 or self.growth < 0:
            raise GFError(-1, "min_cap and growth are not negative")
        if not self.host:
            import torch

            self.ctx, self.torch = ctx or default_context(), torch
            self.dev = torch.device("cuda", torch.cuda.current_device())
            self.tdt = {np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32}
            self.d_status = torch.zeros(4, dtype=torch.int32, device=self.dev)  # apply's two, then move's
        self.b = {name: _Buf(self, _DTYPES[name]) for name in NAMES}
        self.regrows = self.rebuilds = self.flushes = self.launches = 0
        self.rebuild()
        self.rebuilds = 0

    # ------------------------------------------------------------ the journal
    def _clear_journal(self):
        self.j_obs, self.j_slot, self.j_bad = [], [], []
        self.new_kf = self.new_mp = 0

    def log_add_keyframe(self, k):
        """``add_keyframe``: keyframe ``k`` was appended."""
        self.new_kf += 1

    def log_new_map_point(self, p):
        """``new_map_point``: point ``p`` was appended."""
        self.new_mp += 1

    def log_obs_set(self, p, kf, idx):
        """``add_observation``: mObservations[kf] = idx."""
        self.j_obs.append((int(p), OBS_SET, int(kf), int(idx)))

    def log_obs_erase(self, p, kf):
        """``erase_observation``: mObservations.erase(kf)."""
        self.j_obs.append((int(p), OBS_ERASE, int(kf), 0))

    def log_slot(self, kf, idx, value):
        """``add_map_point`` / ``erase_map_point_match``: one slot written."""
        self.j_slot.append((int(kf), int(idx), int(value)))

    def log_set_bad(self, p, obs):
        """``set_bad_point``: the row cleared, the flag set, -1 in every slot
        the observations ``obs`` named."""
        self.j_obs.append((int(p), OBS_CLEAR, 0, 0))
        self.j_bad.append(int(p))
        self.j_slot.extend((int(kf), int(idx), -1) for kf, idx in obs.items())

    def log_replace(self, a, obs):
        """``replace``: the row of ``a`` cleared, its flag set, and every slot
        its observations ``obs`` named as the map holds it now (the survivor or
        -1); the observations given to the survivor logged themselves."""
        self.j_obs.append((int(a), OBS_CLEAR, 0, 0))
        self.j_bad.append(int(a))
        s = self.map.slots
        self.j_slot.extend((int(kf), int(idx), int(s[kf][idx])) for kf, idx in obs.items())

    @property
    def pending(self) -> int:
        """Journal entries and appends not flushed yet."""
        return len(self.j_obs) + len(self.j_slot) + len(self.j_bad) + self.new_kf + self.new_mp

    # ------------------------------------------------------------ build
    def _cap(self, live):
        live = np.asarray(live, np.int64)
        return np.maximum(self.min_cap, live + (self.growth * live).astype(np.int64))

    @staticmethod
    def _offsets(cap):
        off = np.zeros(len(cap) + 1, np.int64)
        off[1:] = np.cumsum(cap)
        if off[-1] >= 2 ** 31:
            raise GFError(-3, "the observation table exceeds 2^31 entries")
        return off.astype(np.int32)

    @staticmethod
    def _xy(kps):
        return np.stack([kps["x"], kps["y"]], axis=1).astype(np.float32).reshape(-1)

    def rebuild(self):
        """The tables built from ``culling_tables(map)`` (the constructor's
        path, and flush's when a row outgrows MT_ROW); the journal is dropped."""
        from .localmapping import culling_tables

        m = self.map
        kf_off, octave, slots, mp_bad, obs_off, obs_gkp, _ = culling_tables(m)
        live = np.diff(obs_off).astype(np.int32)
        off = self._offsets(self._cap(live))
        g = np.full(int(off[-1]), -1, np.int32)
        row = np.repeat(np.arange(len(live)), live)
        g[off[row] + (np.arange(len(obs_gkp)) - obs_off[row])] = obs_gkp
        xy = np.concatenate([np.zeros(0, np.float32)] + [self._xy(k) for k in m.kf_kps])
        for name, a in zip(NAMES, (kf_off, octave, slots, xy, mp_bad, off, g)):
            self.b[name].set(a)
        self.h_kf_off, self.h_obs_off, self.live = kf_off.astype(np.int64), off, live
        self.nkf, self.nmp = m.nkf, len(m.mps)
        self._clear_journal()
        self.rebuilds += 1
        if not self.host:
            self.torch.cuda.current_stream().synchronize()

    # ------------------------------------------------------------ flush
    def flush(self) -> None:
        """The tables brought up to the map: (1) the new keyframes' ``slots``,
        ``octave`` and ``kp_xy`` rows and ``kf_off`` entries appended; (2) the
        new points' rows appended, ``min_cap`` entries of -1 each; (3) when a
        touched row needs more than its capacity, new capacities for all rows
        from the live mirror and one ``gf_map_tables_move_dev``; (4) one
        ``gf_map_tables_apply_dev`` for the journal. The torch copies run on
        torch's stream and are waited for before the kernels go to the
        context's stream. A nonzero status raises; a row that may pass MT_ROW
        entries on the way makes the whole set be rebuilt instead."""
        if not self.pending:
            return
        self.flushes += 1
        self._append_new()
        slot_g, slot_v, bad_p, row_ids, row_op_off, ops, counts = self.journal_arrays()
        final = None
        if len(row_ids):
            final = np.fromiter((len(self.map.obs[p]) for p in row_ids), np.int32, len(row_ids))
            live = self.live[row_ids]
            if np.any(live.astype(np.int64) + counts > MT_ROW) or np.any(final > MT_ROW):
                self.rebuild()
                return
            # (3)
            if np.any(final > self.h_obs_off[row_ids + 1] - self.h_obs_off[row_ids]):
                need = self.live.copy()
                need[row_ids] = np.maximum(live, final)  # what the row holds until the apply, and what it ends with
                self._regrow(self._offsets(self._cap(need)))
        # (4)
        status = self._apply(slot_g, slot_v, bad_p, row_ids, row_op_off, ops)
        if np.any(status != 0):
            raise GFError(-1, f"resident tables: journal not applied cleanly, status {status.tolist()} "
                              "(rows without room, ops out of range, rows lost by the regrow)")
        if final is not None:
            self.live[row_ids] = final
        self._clear_journal()

    def _append_new(self):
        """Steps (1) and (2) of :meth:`flush`."""
        m = self.map
        if self.nkf + self.new_kf != m.nkf or self.nmp + self.new_mp != len(m.mps):
            raise GFError(-1, "the map grew past its resident tables without logging it")
        for k in range(self.nkf, m.nkf):
            kps = m.kf_kps[k]
            if len(kps) > MAX_KEYPOINTS:
                raise GFError(-3, "at most 4096 keypoints per keyframe")
            self.b["octave"].append(kps["octave"].astype(np.uint8))
            self.b["slots"].append(m.slots[k])
            self.b["kp_xy"].append(self._xy(kps))
            self.h_kf_off = np.append(self.h_kf_off, self.h_kf_off[-1] + len(kps))
            self.b["kf_off"].append(self.h_kf_off[-1:])
        self.nkf, self.new_kf = m.nkf, 0
        k = len(m.mps) - self.nmp
        if k:
            off = self._offsets(np.concatenate([np.diff(self.h_obs_off), np.full(k, self.min_cap, np.int64)]))
            self.b["mp_bad"].append(m.mp_bad[self.nmp:].astype(np.uint8))
            self.b["obs_off"].append(off[self.nmp + 1:])
            self.b["obs_gkp"].append(np.full(k * self.min_cap, -1, np.int32))
            self.h_obs_off, self.live = off, np.concatenate([self.live, np.zeros(k, np.int32)])
            self.nmp, self.new_mp = len(m.mps), 0

    def journal_arrays(self):
        """The journal as the arrays ``gf_map_tables_apply`` takes, after the
        appends: the last write per slot (``slot_g``, ``slot_v``), the distinct
        bad points, and the observation ops stable-sorted by point
        (``row_ids``, ``row_op_off``, ``ops`` [nops, 3]) -> those six and the
        number of ops per touched row."""
        slot_g = slot_v = bad_p = row_ids = np.zeros(0, np.int32)
        ops, counts = np.zeros((0, 3), np.int32), np.zeros(0, np.int64)
        row_op_off = np.zeros(1, np.int32)
        if self.j_slot:
            s = np.asarray(self.j_slot, np.int64).reshape(-1, 3)
            g = self.h_kf_off[s[:, 0]] + s[:, 1]
            _, first = np.unique(g[::-1], return_index=True)
            keep = len(g) - 1 - first
            slot_g, slot_v = g[keep].astype(np.int32), s[keep, 2].astype(np.int32)
        if self.j_bad:
            bad_p = np.unique(np.asarray(self.j_bad, np.int32))
        if self.j_obs:
            j = np.asarray(self.j_obs, np.int32).reshape(-1, 4)
            j = j[np.argsort(j[:, 0], kind="stable")]
            row_ids, counts = np.unique(j[:, 0], return_counts=True)
            row_op_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
            ops = np.ascontiguousarray(j[:, 1:])
        return slot_g, slot_v, bad_p, row_ids.astype(np.int32), row_op_off, ops, counts

    def _regrow(self, new_off):
        self.regrows += 1
        old_off, old_gkp = self.b["obs_off"], self.b["obs_gkp"]
        noff, ngkp = _Buf(self, np.int32), _Buf(self, np.int32)
        noff.set(new_off)
        ngkp.reserve(int(new_off[-1]))
        if self.host:
            st = self.applier[1](old_off.view(), old_gkp.view(), noff.view(), ngkp.view())
            if int(np.asarray(st).reshape(-1)[0]):
                raise GFError(-1, "resident tables: the regrow lost rows")
        else:
            self.torch.cuda.current_stream().synchronize()  # the uploads ran on torch's stream
            check(lib().gf_map_tables_move_dev(self.ctx.handle, self.nmp, ptr(old_off.a), ptr(old_gkp.a), old_gkp.n,
                                               ptr(noff.a), ptr(ngkp.a), ngkp.n, ptr(self.d_status[2:]),
                                               self.ctx.stream))
            self.ctx.sync()  # the old buffers are released below
            self.launches += 1
        self.b["obs_off"], self.b["obs_gkp"], self.h_obs_off = noff, ngkp, new_off

    def _apply(self, slot_g, slot_v, bad_p, row_ids, row_op_off, ops):
        b = self.b
        if not len(slot_g) + len(bad_p) + len(row_ids):  # appends only
            if not self.host:
                self.torch.cuda.current_stream().synchronize()
            return np.zeros(3, np.int32)
        if self.host:
            st = self.applier[0](b["kf_off"].view(), b["slots"].view(), b["mp_bad"].view(), b["obs_off"].view(),
                                 b["obs_gkp"].view(), slot_g, slot_v, bad_p, row_ids, row_op_off, ops)
            return np.asarray(st, np.int32).reshape(-1)
        parts = [slot_g, slot_v, bad_p, row_ids, row_op_off, ops.reshape(-1)]
        at = np.concatenate([[0], np.cumsum([len(a) for a in parts])])
        d = self.torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(self.dev)  # one upload
        self.torch.cuda.current_stream().synchronize()  # the appends and this upload ran on torch's stream
        p = [ptr(d[int(o):]) for o in at[:-1]]
        check(lib().gf_map_tables_apply_dev(self.ctx.handle, self.nkf, b["slots"].n, ptr(b["kf_off"].a),
                                            ptr(b["slots"].a), self.nmp, ptr(b["mp_bad"].a), ptr(b["obs_off"].a),
                                            ptr(b["obs_gkp"].a), b["obs_gkp"].n, len(slot_g), p[0], p[1], len(bad_p),
                                            p[2], len(row_ids), p[3], p[4], len(ops), p[5], ptr(self.d_status),
                                            self.ctx.stream))
        self.ctx.sync()
        self.launches += 1
        return self.d_status.cpu().numpy()[:3]  # the third is the last regrow's, waited for above

    # ------------------------------------------------------------ what the stages take
    def sizes(self) -> dict:
        """nkf, nkp, nmp and nobs (the used length of ``obs_gkp``, padding included)."""
        return dict(nkf=self.nkf, nkp=self.b["slots"].n, nmp=self.nmp, nobs=self.b["obs_gkp"].n)

    def arrays(self) -> dict:
        """The tables as they are resident (device tensors, or host arrays with
        an applier), cut to their used lengths. Taken after a flush: a flush may
        reallocate."""
        return {name: self.b[name].view() for name in NAMES}

    def download(self) -> dict:
        """Host copies of the tables as of the last flush."""
        if self.host:
            return {name: self.b[name].view().copy() for name in NAMES}
        return {name: self.b[name].view().cpu().numpy() for name in NAMES}

    def host_arrays(self) -> dict:
        """The tables on the host for an injected counter / assembler."""
        return self.arrays() if self.host else self.download()

    def slack(self) -> float:
        """Capacity / live entries of the observation table."""
        return float(self.b["obs_gkp"].n) / max(int(self.live.sum()), 1)

    def check(self) -> None:
        """The resident tables, -1 entries dropped, against ``culling_tables(map)``
        and the mirrors against the tables; raises naming the first differing
        row. Call it after a flush."""
        from .localmapping import culling_tables

        if self.pending:
            raise GFError(-1, "check() needs a flushed journal")
        t, m = self.download(), self.map
        kf_off, octave, slots, mp_bad, obs_off, obs_gkp, _ = culling_tables(m)
        xy = np.concatenate([np.zeros(0, np.float32)] + [self._xy(k) for k in m.kf_kps])
        for name, want in (("kf_off", kf_off), ("octave", octave), ("slots", slots), ("kp_xy", xy), ("mp_bad", mp_bad)):
            got = t[name]
            if got.shape != want.shape or not np.array_equal(got, want):
                n = min(len(got), len(want))
                d = np.nonzero(got[:n] != want[:n])[0]
                raise GFError(-1, f"resident {name} differs from the map at entry {int(d[0]) if len(d) else n}")
        off, g = t["obs_off"], t["obs_gkp"]
        if not np.array_equal(off, self.h_obs_off) or len(off) != len(obs_off) or off[0] != 0 or off[-1] != len(g):
            raise GFError(-1, "resident obs_off differs from its mirror or from the map's point count")
        livemask = g >= 0
        csum = np.concatenate([[0], np.cumsum(livemask)])
        cnt = csum[off[1:]] - csum[off[:-1]]
        row = np.repeat(np.arange(len(cnt)), np.diff(off))
        rank = np.arange(len(g)) - off[row]
        problems = [np.nonzero(cnt != np.diff(obs_off))[0], np.nonzero(cnt != self.live)[0],
                    row[livemask & (rank >= cnt[row])], row[~livemask & (g != -1)]]
        if not any(len(p) for p in problems):
            d = np.nonzero(g[livemask] != obs_gkp)[0]
            problems.append(row[livemask][d])
        first = [int(p.min()) for p in problems if len(p)]
        if first:
            p = min(first)
            raise GFError(-1, f"resident observation row {p} differs from the map: holds "
                              f"{g[off[p]:off[p + 1]].tolist()}, the map {obs_gkp[obs_off[p]:obs_off[p + 1]].tolist()}, "
                              f"live mirror {int(self.live[p])}")
