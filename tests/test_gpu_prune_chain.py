"""kb_prune and kb_shared_prune on the device, removal by removal, against tests/prune_mirror.py AS BITS.

What defines the bits.  The pruning rule forms no sum (kb_prune.hip's header): per removal one negation, one division, one
product and one addition per coefficient, one product, one division and one subtraction per entry of Kinv.  Mirror.remove_one
performs exactly these IEEE float64 operations in that order (separate NumPy ufuncs, nothing fused; tests/test_prune_mirror.py
pins it to a restatement in Python floats written from the header's seven steps).  So a mirror LOADED WITH THE DEVICE'S OWN
STATE (Mirror.from_state, read from a save_state blob before the first removal) and continued from its own state from then on
must hold, after every removal, the bytes the device holds.  No comparison in this file carries a tolerance.

Per removal, each under its own stage name in the failure message: the victim (read off the landmark arrays), the
coefficients, every stored entry of Kinv (named by tile (b_i, b_j) and unit of sixteen rows; on shared handles both stored
triangles against the mirror), the landmark rows and the float32 copy of every live slot, the grid-index row, links, heads
and the off-grid count against chains(idx), exact zeros in everything vacated (D0 / E are scratch of the state being
processed: nobody's state), the predict caches dropped on touched dictionaries only, the pruned counters and the work counters
of kb_get_prune_work against their closed forms.

Dictionaries are grown by VecKBRL.fit on prefixes of one random stream per kind of learner (ten state variables: the float32
copy travels with a landmark; three: all sixteen coordinate rows do).  Victims are forced, and state is corrupted, only by
editing a save_state blob and loading it; every corrupted state is one the kernels refuse by design."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_mirror as pm   # noqa: E402
import test_gpu_prune as tp   # noqa: E402
import test_gpu_shared_prune as tsp   # noqa: E402
from ranslice import _lib   # noqa: E402

pytestmark = pytest.mark.gpu

DIMS, N_PRBS = [10, 3], 200
IA, SF = [10, 5], [3, 2]
ROW_CO, ROW_KF, ROW_DS, ROW_IDX = 16, 19, 20, 21     # rows of a vector page (kb_kbrl.hip: KB_ROW_*)
KINDS = [False, True]
KIND_IDS = ['agents', 'shared']


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same(what, stage, got, want):
    """got == want as bytes; the failure names the stage and the first element that differs"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, '%s: %s: %s %s against %s %s' % (what, stage, got.shape, got.dtype,
                                                                                                 want.shape, want.dtype)
    if got.tobytes() != want.tobytes():
        u = {8: np.uint64, 4: np.uint32}[got.dtype.itemsize]
        at = np.argwhere(got.view(u) != want.view(u))[0].tolist()
        raise AssertionError('%s: %s: first difference at %s, device %r, mirror %r' % (what, stage, at, got[tuple(at)], want[tuple(at)]))


def _victim(before, after, what):
    """the slot one removal took its landmark from, read off the landmark rows before and after it: the last landmark moved
    into it.  Rows are compared as bits: the rows beyond a learner's own coordinates (three state variables: rows 4..15) are
    never written by anybody before a prune clears them, travel with the landmark as they are and may hold anything, NaN
    included"""
    m = len(before)
    assert len(after) == m - 1, '%s: victim: %d rows after %d' % (what, len(after), m)
    b, a = (np.ascontiguousarray(x).view(np.uint64) for x in (before, after))
    moved = np.nonzero((a != b[:m - 1]).any(axis=1))[0]
    if len(moved) == 0:
        return m - 1
    assert len(moved) == 1 and (a[moved[0]] == b[m - 1]).all(), '%s: victim: slots %s changed' % (what, moved.tolist())
    return int(moved[0])


def _zeros(what, stage, got):
    assert not np.ascontiguousarray(got).view(np.uint8).any(), '%s: %s' % (what, stage)


# ------------------------------------------------------------------ a handle of either kind as a window on its device state
class _Dev:
    def __init__(self, h):
        self.h = h
        self.shared = bool(h.cfg.shared_dictionary)
        self.S = h.S
        self.nd = h.S if self.shared else h.n_envs * h.S
        self.name = 'kb_shared_prune' if self.shared else 'kb_prune'

    def views(self, blob=None):
        """the arrays of a checkpoint blob (default: one taken now); the blob's sizes must be the handle's"""
        blob = self.h.save_state() if blob is None else blob
        if self.shared:
            return tsp._views(self.h, blob)
        v = tp._blob_views(self.h, blob)
        # fver [T] int32 of a per-replica handle: behind f32bad come F [T][256] float64 and fstate [T][16] float32 (kb_api.hip,
        # the allocation order)
        T = self.nd
        at = lambda a: a.__array_interface__['data'][0]
        o = at(v['f32bad']) - at(blob) + 4 * T + 8 * 256 * T + 4 * 16 * T
        assert 0 < o and o + 4 * T <= blob.size
        v['fver'] = blob[o:o + 4 * T].view(np.int32)
        return v

    def eMBB(self, d):
        return self.h.dims[d % self.S] == 10

    def tile(self, v, d, bi, bj):
        return (tsp._tile if self.shared else tp._tile)(v, d, bi, bj)

    def stored(self, nb):
        """the tiles the handle stores: the lower block triangle (diagonal tiles whole), or the block square"""
        return [(bi, bj) for bi in range(nb) for bj in range(nb if self.shared else bi + 1)]

    def prune(self, t):
        return self.h.shrink(t) if self.shared else self.h.prune(t)

    def caches(self, v, d):
        """the cache guards of dictionary d -- m_last and kf_owner of kb_predict, fver of the stored select scores --: of its
        task, or of the n_envs tasks of its slice"""
        if self.shared:
            return dict(m_last=v['m_last'][:, d], fver=v['fver'][:, d], kf_owner=v['kf_owner'][d:d + 1])
        return dict(m_last=v['m_last'][d:d + 1], fver=v['fver'][d:d + 1], kf_owner=v['kf_owner'][d:d + 1])

    def units(self, m):
        """units of sixteen rows that hold rows in one downdate of a dictionary of m landmarks (the closed forms)"""
        nb = (m + 63) // 64
        rows_last = m - 64 * (nb - 1)
        full = (nb - 1) * nb * 4 if self.shared else (nb - 1) * nb // 2 * 4
        return full + nb * ((rows_last + 15) // 16)

    def line(self, m):
        """units the plan lays out for it: four per stored tile"""
        nb = (m + 63) // 64
        return nb * nb * 4 if self.shared else nb * (nb + 1) // 2 * 4

    def work(self):
        w = (C.c_uint64 * 2)()
        self.h._check(self.h.L.kb_get_prune_work(self.h.h, w))
        return int(w[0]), int(w[1])


def _pages(v, d, nb):
    """the rows of the first nb vector pages of dictionary d, by slot: rows [64 nb, 16] (the coordinate rows), co, kf, ds
    [64 nb], idx, link [64 nb] int32 and f32 [64 nb, 10], rows 11..15 read as the float32 copy of ten coordinates"""
    P = np.stack([tp._page(v, d, b) for b in range(nb)])                      # [nb, 30, 64]
    by_slot = lambda a: np.ascontiguousarray(np.moveaxis(a, 1, 2)).reshape(nb * 64, a.shape[1])
    ix = np.ascontiguousarray(P[:, ROW_IDX]).view(np.int32).reshape(nb, 128)
    f32 = np.ascontiguousarray(P[:, 11:16]).view(np.float32).reshape(nb, 10, 64)
    return dict(all=P, rows=by_slot(P[:, :16]), co=P[:, ROW_CO].reshape(-1), kf=P[:, ROW_KF].reshape(-1), ds=P[:, ROW_DS].reshape(-1),
                idx=ix[:, :64].reshape(-1), link=ix[:, 64:].reshape(-1), f32=by_slot(f32))


def _load(dev, v, d):
    """a mirror of dictionary d as the device holds it: Kinv from the lower block triangle and its transpose"""
    m = int(v['m'][d])
    nb = (m + 63) // 64
    pg = _pages(v, d, nb)
    A = np.zeros((nb * 64, nb * 64))
    for bi in range(nb):
        for bj in range(bi + 1):
            T = dev.tile(v, d, bi, bj)
            A[64 * bi:64 * bi + 64, 64 * bj:64 * bj + 64] = T
            if bi != bj:
                A[64 * bj:64 * bj + 64, 64 * bi:64 * bi + 64] = T.T
    P = A[:m, :m].copy()
    assert _bits(P) == _bits(P.T), 'dictionary %d: the diagonal tiles are not symmetric' % d
    return pm.Mirror.from_state(pg['rows'][:m, :11 if dev.eMBB(d) else 16], pg['co'][:m], P, pg['idx'][:m])


def _hold(dev, v, d, mr, m0, what):
    """dictionary d of snapshot v against its mirror, stage by stage; m0 = its size when the mirror was loaded: everything
    between the mirror's size and m0 has been vacated"""
    m = mr.m
    assert int(v['m'][d]) == m, '%s: size: device %d, mirror %d' % (what, int(v['m'][d]), m)
    nb0 = (m0 + 63) // 64
    pg = _pages(v, d, nb0)
    nr = 11 if dev.eMBB(d) else 16
    _same(what, 'coefficients', pg['co'][:m], mr.c)
    _same(what, 'landmark rows', pg['rows'][:m, :nr], mr.L)
    if dev.eMBB(d):
        _same(what, 'float32 copy of the live slots', pg['f32'][:m], mr.L[:, :10].astype(np.float32))
    _same(what, 'grid index', pg['idx'][:m], mr.idx.astype(np.int32))
    head, link = pm.chains(mr.idx)
    _same(what, 'links', pg['link'][:m], link.astype(np.int32))
    _same(what, 'head', v['head'][d], head.astype(np.int32))
    assert int(v['offgrid'][d]) == int((mr.idx < 0).sum()), '%s: offgrid' % what
    # every stored entry that ever was Kinv's: the mirror's P, zeros around it
    E = np.zeros((nb0 * 64, nb0 * 64))
    E[:m, :m] = mr.P
    for bi, bj in dev.stored(nb0):
        r, c = min(64, m0 - 64 * bi), min(64, m0 - 64 * bj)
        T = np.ascontiguousarray(dev.tile(v, d, bi, bj)[:r, :c]).view(np.uint64)
        W = np.ascontiguousarray(E[64 * bi:64 * bi + r, 64 * bj:64 * bj + c]).view(np.uint64)
        if (T != W).any():
            row = int(np.nonzero((T != W).any(axis=1))[0][0])
            col = int(np.nonzero(T[row] != W[row])[0][0])
            raise AssertionError('%s: Kinv tile (%d, %d), unit %d: row %d column %d of the tile (entry [%d][%d], %s), device %r, mirror %r'
                                 % (what, bi, bj, row // 16, row, col, 64 * bi + row, 64 * bj + col,
                                    'live' if 64 * bi + row < m and 64 * bj + col < m else 'vacated',
                                    T[row, col:col + 1].view(np.float64)[0], W[row, col:col + 1].view(np.float64)[0]))
    # what was vacated (beyond Kinv, which the zeros around P cover)
    _zeros(what, 'vacated coefficients', pg['co'][m:m0])
    _zeros(what, 'vacated landmark rows', pg['rows'][m:m0, :nr])
    if dev.eMBB(d):
        _zeros(what, 'vacated float32 copy', pg['f32'][m:m0])
    _zeros(what, 'vacated K_f', pg['kf'][m:m0])
    _zeros(what, 'vacated d*', pg['ds'][m:m0])
    _zeros(what, 'vacated grid index', pg['idx'][m:m0])
    _zeros(what, 'vacated links', pg['link'][m:m0])


def _untouched(dev, before, after, d, m0, what):
    """every page (all thirty rows) and every stored tile of dictionary d holds the bytes it held"""
    assert int(after['m'][d]) == int(before['m'][d]), '%s: size' % what
    nb0 = (m0 + 63) // 64
    if nb0:
        _same(what, 'untouched pages', _pages(after, d, nb0)['all'], _pages(before, d, nb0)['all'])
    for bi, bj in dev.stored(nb0):
        _same(what, 'untouched Kinv tile (%d, %d)' % (bi, bj), dev.tile(after, d, bi, bj), dev.tile(before, d, bi, bj))
    _same(what, 'untouched head', after['head'][d], before['head'][d])
    assert int(after['offgrid'][d]) == int(before['offgrid'][d]), '%s: untouched offgrid' % what


class _Run:
    """a handle, the last snapshot of its state and one mirror per dictionary, loaded from the device when the run begins and
    never again; the pruned counters and the work counters it must show"""

    def __init__(self, h, only=None):
        self.dev = dev = _Dev(h)
        self.v = dev.views()
        self.mirrors, self.m0 = {}, {}
        for d in range(dev.nd):
            self.m0[d] = int(self.v['m'][d])
            if self.m0[d] and (only is None or d in only):
                self.mirrors[d] = _load(dev, self.v, d)
                _hold(dev, self.v, d, self.mirrors[d], self.m0[d], 'dictionary %d at the start' % d)
                for name, c in dev.caches(self.v, d).items():      # armed, every task: "dropped" must be the prune's doing
                    assert (c != -1).all(), 'dictionary %d at the start: %s is not armed: %s' % (d, name, c)
        self.only = only
        self.pruned = np.zeros(dev.nd, dtype=np.int64)
        self.units, self.launches = dev.work()

    def call(self, t, what, expect=None, stops=None):
        """one prune call to target t, every dictionary held to its mirror afterwards.  expect: the whole message of the
        RS_ESTATE the call must answer with; stops: {dictionary: removals it completes}, where that is not size - t
        -> {dictionary: the mirror's removal records}.  The victim is read off the landmark arrays where the call makes one
        removal of a dictionary; where it makes several (dictionary 1 of the status-3 case: three) the dictionary is compared
        in its end state only, whose landmark rows by slot still imply the victims"""
        dev, prev = self.dev, self.v
        if expect is None:
            removed = dev.prune(t)
        else:
            with pytest.raises(_lib.RanSliceError) as ei:
                dev.prune(t)
            assert ei.value.code == _lib.RS_ESTATE, '%s: code %d' % (what, ei.value.code)
            assert str(ei.value) == 'libranslice error %d: %s' % (_lib.RS_ESTATE, expect), '%s: message %r' % (what, str(ei.value))
            removed = None
        self.v = v = dev.views()
        logs, total, todo = {}, 0, {}
        for d in range(dev.nd):
            mb = int(prev['m'][d])
            k = max(mb - t, 0)
            if stops and d in stops:
                k = stops[d]
            todo[d] = (mb, k)
            total += k
            self.pruned[d] += k
            w = '%s, dictionary %d (%d landmarks -> %d)' % (what, d, mb, mb - k)
            if d in self.mirrors and k:
                mr = self.mirrors[d]
                logs[d] = [mr.remove_one() for _ in range(k)]
                assert all(st['diag_ok'] for st in logs[d]), w
                if k == 1:        # the victim, read off the landmark arrays
                    nb, nr = (mb + 63) // 64, 11 if dev.eMBB(d) else 16
                    assert int(v['m'][d]) == mb - 1, '%s: size' % w
                    got = _victim(_pages(prev, d, nb)['rows'][:mb, :nr], _pages(v, d, nb)['rows'][:mb - 1, :nr], w)
                    assert got == logs[d][0]['slot'], '%s: victim: device slot %d, mirror slot %d' % (w, got, logs[d][0]['slot'])
                _hold(dev, v, d, mr, self.m0[d], w)
            elif k == 0:
                _untouched(dev, prev, v, d, self.m0[d] if d in self.mirrors else 0, w)
            else:
                assert int(v['m'][d]) == mb - k, '%s: size' % w
            now, was = dev.caches(v, d), dev.caches(prev, d)
            for name in now:
                if k:
                    assert (now[name] == -1).all(), '%s: %s of a touched dictionary: %s' % (w, name, now[name])
                else:
                    assert np.array_equal(now[name], was[name]), '%s: %s of an untouched dictionary moved' % (w, name)
        if removed is not None:
            assert removed == total, '%s: removed %d, expected %d' % (what, removed, total)
        assert np.array_equal(dev.h.pruned().reshape(-1), self.pruned), '%s: pruned() %s' % (what, dev.h.pruned().reshape(-1))
        # the work counters: per round, the units that hold rows over the dictionaries still active in it
        for i in range(max(k for _, k in todo.values())):
            self.units += sum(dev.units(mb - i) for mb, k in todo.values() if k > i)
            self.launches += 1
        assert dev.work() == (self.units, self.launches), '%s: kb_get_prune_work %s, closed forms %s' % (what, dev.work(), (self.units, self.launches))
        return logs


# ------------------------------------------------------------------ growing the dictionaries
_cache = {}


@pytest.fixture(scope='module', autouse=True)
def _release_handles():
    """the base handles of the forced cases live as long as this module's tests, no longer"""
    yield
    for key, value in list(_cache.items()):
        if key[0] == 'base':
            value[0].close()
    _cache.clear()


def _streams():
    if 'streams' not in _cache:
        rng = np.random.default_rng(77)
        x0, y0 = tp._random_stream(rng, 11, 1500, offgrid_every=17)
        x1, y1 = tp._random_stream(rng, 4, 1600, offgrid_every=13, spread=4.0)   # (three state variables: spread out)
        _cache['streams'] = (x0, y0, x1, y1)
    return _cache['streams']


def _curves(dev_build):
    """the size of each kind's dictionary after every sample of its stream"""
    key = ('curves', dev_build)
    if key not in _cache:
        from ranslice.kbrl_dev import VecKBRL
        x0, y0, x1, y1 = _streams()
        ag = VecKBRL(1, DIMS, N_PRBS, capacity=512, pool_bytes=64 << 20)
        ag.reset([IA], [SF])
        r = ag.fit([(0, 0), (0, 1)], [x0, x1], [y0, y1])
        _cache[key] = [np.asarray(r['m'][s]).copy() for s in (0, 1)]
        ag.close()
    return _cache[key]


def _grow(sizes10, sizes3, capacity, dev_build=False):
    """a per-replica handle whose agents e hold sizes10[e] landmarks of ten state variables and sizes3[e] of three (none where
    the list is shorter), grown by kb_fit on the shortest prefixes of the two streams that reach them.  Then one
    kb_select_action and, for every learner that holds landmarks, one kb_predict: fver, m_last and kf_owner are armed"""
    from ranslice.kbrl_dev import VecKBRL
    x0, y0, x1, y1 = _streams()
    curves = _curves(dev_build)
    n = max(len(sizes10), len(sizes3))
    ag = VecKBRL(n, DIMS, N_PRBS, capacity=capacity, pool_bytes=64 << 20)
    ag.reset([IA] * n, [SF] * n)
    learners, X, Y = [], [], []
    for s, sizes, xs, ys in ((0, sizes10, x0, y0), (1, sizes3, x1, y1)):
        for e, size in enumerate(sizes):
            assert curves[s].max() >= size, (s, size, curves[s].max())
            cut = int(np.argmax(curves[s] >= size)) + 1
            learners.append((e, s))
            X.append(xs[:cut])
            Y.append(ys[:cut])
    ag.fit(learners, X, Y)
    got = ag.dictionary_sizes()
    ag.select_action(np.full((n, sum(DIMS)), 0.25, dtype=np.float32))     # (arms fver of every task: the stored select scores)
    for (e, s), x in zip(learners, X):
        assert got[e, s] == (sizes10, sizes3)[s][e], (e, s, got[e, s])
        ag.predict(e, s, np.full(DIMS[s] + 1, 0.25))
    return ag


def _base(size, shared, dev_build=False):
    """-> (handle, pristine blob) of the two dictionaries the forced cases work on: size landmarks of ten state variables and
    193 (size 193) or 130 (size 321) of three; shared: the same two through to_shared, three replicas.  Every case begins by
    loading an edited copy of the blob.  dev_build: handles of the test build, made while RANSLICE_DEV_BUILD is set"""
    key = ('base', size, shared, dev_build)
    if key not in _cache:
        src_key = ('base', size, False, dev_build)
        if src_key not in _cache:
            ag = _grow((size,), (193 if size == 193 else 130,), 256 if size == 193 else 384, dev_build=dev_build)
            _cache[src_key] = (ag, ag.save_state())
        if shared:
            X = _cache[src_key][0]
            X.load_state(_cache[src_key][1])
            sh = X.to_shared(0, 3)
            for e in range(3):                     # m_last of EVERY task of a slice; kf_owner names the last one
                for s in range(2):
                    sh.predict(e, s, np.full(DIMS[s] + 1, 0.25))
            # fver: no kernel of a shared handle stores anything but -1 there today (the stored select scores are the
            # per-replica path's), so it is armed where every other state of these cases is forced: in the blob.  The value
            # can equal no dictionary version
            blob = sh.save_state()
            _Dev(sh).views(blob)['fver'][:] = 1 << 20
            _cache[key] = (sh, blob)
    h, blob = _cache[key]
    h.load_state(blob)
    return h, blob


def _edited(h, blob, edit):
    """load a copy of `blob` that edit(dev, views) has changed -> a _Dev of the handle"""
    dev = _Dev(h)
    blob = blob.copy()
    edit(dev, dev.views(blob))
    h.load_state(blob)
    return dev


def _set_co(v, d, j, value):
    tp._page(v, d, j >> 6)[ROW_CO, j & 63] = value


def _set_diag(dev, v, d, j, value):
    dev.tile(v, d, j >> 6, j >> 6)[j & 63, j & 63] = value


# ------------------------------------------------------------------ (a) the size ladder, natural victims; (f) its counters
LADDER10, LADDER3 = (66, 81, 130, 193, 258, 321), (66, 130, 193)


def test_size_ladder_natural_victims():
    """One handle holds dictionaries of 66, 81, 130, 193, 258 and 321 landmarks of ten state variables and of 66, 130 and 193 of
    three (and three empty ones).  prune(t) for t = 320 down to 64, one removal per call and dictionary: every m from 321 to 65
    is passed -- odd m (the 16-byte store that keeps its first half), last block rows of 1 .. 64 live rows, 2 .. 6 blocks.
    Every dictionary is held to its mirror after EVERY call, the untouched ones to their own earlier bytes, and the work
    counters to their closed forms; the mirrors are loaded once, before the first removal."""
    ag = _grow(LADDER10, LADDER3, 384)
    run = _Run(ag)
    assert len(run.mirrors) == 9 and run.dev.work() == (0, 0)
    victims = set()
    for t in range(320, 63, -1):
        logs = run.call(t, 'ladder, prune(%d)' % t)
        assert len(logs) == sum(m > t for m in LADDER10 + LADDER3)
        for d, steps in logs.items():
            victims.add('last' if steps[0]['slot'] == t else 'block %d of %d' % (steps[0]['slot'] >> 6, (t + 64) >> 6))
    print('ladder: victims met:', sorted(victims), 'work', run.dev.work())
    assert list(ag.dictionary_sizes().reshape(-1)) == [64, 64, 64, 64, 64, 64, 64, 0, 64, 0, 64, 0]
    assert run.launches == 257 and run.units > 0
    ag.close()


# ------------------------------------------------------------------ (b) forced victims
@pytest.mark.parametrize('shared', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('r', [192, 191, 0, 63, 64, 128, 129])
def test_forced_victim(r, shared):
    """a zero coefficient at slot r of both 193-landmark dictionaries: r = the last slot (nothing moves), the last slot's
    neighbour, and victims in each block on both sides of the block seams while the last slot lies in block 3"""
    h, blob = _base(193, shared)

    def edit(dev, v):
        for d in (0, 1):
            _set_co(v, d, r, 0.0)

    _edited(h, blob, edit)
    run = _Run(h)
    logs = run.call(192, 'victim forced at slot %d' % r)
    assert [logs[d][0]['slot'] for d in (0, 1)] == [r, r] and all(logs[d][0]['key'] == 0.0 for d in (0, 1))


# ------------------------------------------------------------------ (c) ties
ZEROS = {'5, 70, 261, 300: one thread, other lanes, other waves': (5, 70, 261, 300),
         '200, 300: the lower slot in the later wave': (200, 300),
         '40, 266: the lower slot in the higher lane': (40, 266)}


@pytest.mark.parametrize('shared', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('case', list(ZEROS))
def test_ties_of_zero_keys(case, shared):
    """zero coefficients at several slots of the 321-landmark dictionary (thread = slot mod 256, lane = slot mod 64): as many
    removals, one per call; the victims are the mirror's -- the lowest slot among the equal keys every time"""
    slots = ZEROS[case]
    h, blob = _base(321, shared)
    _edited(h, blob, lambda dev, v: [_set_co(v, 0, j, 0.0) for j in slots])
    run = _Run(h)
    seen = []
    for i in range(len(slots)):
        st = run.call(320 - i, 'tie of zero keys, removal %d' % i)[0][0]
        assert st['key'] == 0.0 and (st['gap'] == 0.0 or i == len(slots) - 1)
        seen.append(st['id'])
    assert seen == sorted(slots)      # (ids: the slots the landmarks held when the mirror was loaded)


@pytest.mark.parametrize('shared', KINDS, ids=KIND_IDS)
def test_tie_of_two_equal_nonzero_keys(shared):
    """slots 40 and 266 of the 321-landmark dictionary with the same coefficient 1e-9 and the same diagonal entry (the larger
    of the two copied to the other slot: raising a diagonal entry keeps Kinv positive definite): two equal keys that are not
    zero and lie below every other; slot 40 leaves first, then the other"""
    a, b = 40, 266
    h, blob = _base(321, shared)

    def edit(dev, v):
        P = _load(dev, v, 0).P
        for j in (a, b):
            _set_co(v, 0, j, 1e-9)
            _set_diag(dev, v, 0, j, max(P[a, a], P[b, b]))

    _edited(h, blob, edit)
    run = _Run(h)
    mr = run.mirrors[0]
    keys = (mr.c * mr.c) / np.diag(mr.P)
    assert keys[a] == keys[b] == keys.min() > 0.0 and (keys == keys.min()).sum() == 2
    first = run.call(320, 'two equal keys, first removal')[0][0]
    second = run.call(319, 'two equal keys, second removal')[0][0]
    assert (first['slot'], first['gap'], second['id']) == (a, 0.0, b)


# ------------------------------------------------------------------ (d) refusals and the mid-way stop
BAD = {'diagonal -1.0': ('diag', -1.0), 'diagonal 0.0': ('diag', 0.0), 'diagonal +inf': ('diag', np.inf), 'diagonal NaN': ('diag', np.nan),
       'coefficient inf': ('co', np.inf), 'coefficient NaN': ('co', np.nan)}
REFUSED = ('%s: %d dictionaries hold a Kinv diagonal entry that is not finite and positive (%d left untouched, %d stopped after completed '
           'removals); the others were pruned')


def _stop_after_one(dev, v, d, r):
    """edit dictionary d of the blob behind v so that it completes exactly one removal: a zero coefficient makes slot r the
    first victim, and the diagonal entry of the slot j with the largest |P[j][r]| becomes half of P[j][r]^2 / P[r][r] --
    positive now, negative after the first downdate, which the second round's choose kernel refuses (status 3)"""
    P = _load(dev, v, d).P
    col = np.abs(P[:, r])
    col[r] = 0.0
    j = int(np.argmax(col))
    half = 0.5 * ((P[j, r] * P[j, r]) / P[r, r])
    assert 0.0 < half < P[j, j] and np.isfinite(half)
    _set_co(v, d, r, 0.0)
    _set_diag(dev, v, d, j, half)


@pytest.mark.parametrize('shared', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('case', list(BAD))
def test_refused_dictionary_is_untouched(case, shared):
    """Kinv[5][5] or the coefficient of slot 5 of dictionary 0 holds a value the choose kernel refuses: status 2 -- the call
    answers RS_ESTATE with the whole message, dictionary 0 holds every byte it held (pages, tiles, chains, caches, counter),
    dictionary 1 of the handle loses its landmark as its mirror does"""
    where, value = BAD[case]
    h, blob = _base(193, shared)
    dev = _edited(h, blob, lambda dev, v: _set_diag(dev, v, 0, 5, value) if where == 'diag' else _set_co(v, 0, 5, value))
    run = _Run(h)
    logs = run.call(192, case, expect=REFUSED % (dev.name, 1, 1, 0), stops={0: 0})
    assert list(logs) == [1] and list(h.dictionary_sizes().reshape(-1)) == [193, 192] and list(h.pruned().reshape(-1)) == [0, 1]


@pytest.mark.parametrize('shared', KINDS, ids=KIND_IDS)
def test_stops_after_one_completed_removal(shared):
    """Status 3.  Slot r = 10 of dictionary 0 is the first victim (zero coefficient), and the diagonal entry of the slot j with
    the largest |P[j][r]| is set to half of P[j][r]^2 / P[r][r]: positive now, negative after the first downdate.  prune(m - 3):
    dictionary 0 completes exactly one removal -- the mirror's, as bytes --, stands at m - 1 with chains rebuilt and caches
    dropped, pruned() is 1, the call answers RS_ESTATE "0 left untouched, 1 stopped after completed removals", and dictionary
    1 reaches its target"""
    r, m = 10, 193
    h, blob = _base(193, shared)
    dev = _edited(h, blob, lambda dev, v: _stop_after_one(dev, v, 0, r))
    run = _Run(h)
    logs = run.call(m - 3, 'stop after one removal', expect=REFUSED % (dev.name, 1, 0, 1), stops={0: 1})
    assert logs[0][0]['slot'] == r and len(logs[0]) == 1 and len(logs[1]) == 3
    diag = np.diag(run.mirrors[0].P)
    assert (diag <= 0.0).sum() == 1, 'the second round must meet exactly one diagonal entry that is not positive'
    assert list(h.dictionary_sizes().reshape(-1)) == [m - 1, m - 3] and list(h.pruned().reshape(-1)) == [1, 3]


# ------------------------------------------------------------------ (g) the shared ladder
def test_shared_ladder():
    """SharedVecKBRL.shrink(t) for t = 192 down to 64 on dictionaries of 193 landmarks of ten and of three state variables:
    after every call both stored triangles, pages, chains, caches and counters against the mirrors"""
    h, blob = _base(193, True)
    run = _Run(h)
    for t in range(192, 63, -1):
        logs = run.call(t, 'shared ladder, shrink(%d)' % t)
        assert sorted(logs) == [0, 1]
    assert list(h.dictionary_sizes()) == [64, 64] and run.launches == 129


# ------------------------------------------------------------------ (e) stretches longer than a unit, across dictionaries
SOURCES = (255, 300, 383, 440)      # 4, 5, 6 and 7 blocks


def _prune_grid(h):
    h.L.kb_dev_get_prune_grid.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    h.L.kb_dev_get_prune_grid.restype = C.c_int
    g = C.c_int32(-1)
    h._check(h.L.kb_dev_get_prune_grid(h.h, C.byref(g)))
    return int(g.value)


def _set_prune_grid(h, grid):
    h.L.kb_dev_set_prune_grid.argtypes = [C.c_void_p, C.c_int32]
    h.L.kb_dev_set_prune_grid.restype = C.c_int
    return h.L.kb_dev_set_prune_grid(h.h, grid)


def test_stretches_across_dictionaries():
    """Four source dictionaries of 4, 5, 6 and 7 blocks, forked in a shuffled order into one handle, as many copies as make one
    round's work line at least three times as long as the waves prune_downdate_kernel is launched with (its grid: host state,
    read through kb_dev_get_prune_grid of the test build).  ONE removal per dictionary, all in the one round that holds them
    all: prune(254) takes the copies of the smallest source (255 landmarks) to the target, and the three larger sources are
    edited (_stop_after_one) so that their copies stop after their first removal -- the call answers RS_ESTATE with the
    count.  Every copy is held to the mirror of its source (whose bytes it is shown to hold before the call), so a unit that
    no wave takes shows as the Kinv tile and unit it is.  The stretches of that round, computed from the plan's prefix sums
    and the grid as wave_share does, are all at least three units long, at least one crosses from one dictionary into the
    next and at least one begins inside a tile (u0 & 3 != 0).  The work counters equal the closed forms of that round."""
    from ranslice.kbrl_dev import VecKBRL, fork_pool_bytes
    target = SOURCES[0] - 1
    forced = {1: 7, 2: 100, 3: 300}                      # source -> its first victim
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('RANSLICE_DEV_BUILD', '1')
        src = _grow(SOURCES, (), 448, dev_build=True)
        sdev = _edited(src, src.save_state(), lambda dev, v: [_stop_after_one(dev, v, 2 * e, r) for e, r in forced.items()])
        assert src.prune(448) == 0                       # nothing to do: the call only chooses the grid
        grid = _prune_grid(src)
        waves = 4 * grid
        per_set = sum(sdev.line(m) for m in SOURCES)
        sets = -(-3 * waves // per_set)
        index = np.repeat(np.arange(4, dtype=np.int32), sets)
        np.random.default_rng(4).shuffle(index)
        n = len(index)
        print('grid %d workgroups, %d waves; %d copies of each source, %d dictionaries' % (grid, waves, sets, n))
        assert 64 <= n <= 1024, n
        sizes = np.array(SOURCES)[index]
        big = VecKBRL(n, DIMS, N_PRBS, capacity=448, pool_bytes=fork_pool_bytes(sizes) + (64 << 20))
        big.fork_from(src, index)
        big.select_action(np.full((n, sum(DIMS)), 0.25, dtype=np.float32))   # (a fork drops the stored select scores: fver again)
        dev = _Dev(big)
        sv, v0 = sdev.views(), dev.views()
        want = {e: _load(sdev, sv, 2 * e) for e in range(4)}
        for j in range(n):                               # every copy holds its source's bytes: the source's mirror is its own
            e, d = int(index[j]), 2 * j
            nb = (SOURCES[e] + 63) // 64
            assert int(v0['m'][d]) == SOURCES[e] and int(v0['m'][d + 1]) == 0
            _same('copy %d' % j, 'pages of the source', _pages(v0, d, nb)['all'][:, :17], _pages(sv, 2 * e, nb)['all'][:, :17])
            _same('copy %d' % j, 'grid index and links of the source', _pages(v0, d, nb)['all'][:, ROW_IDX], _pages(sv, 2 * e, nb)['all'][:, ROW_IDX])
            for bi, bj in dev.stored(nb):
                _same('copy %d' % j, 'tile (%d, %d) of the source' % (bi, bj), dev.tile(v0, d, bi, bj), sdev.tile(sv, 2 * e, bi, bj))
            assert int(v0['m_last'][d]) == SOURCES[e]    # (the source's armed predict cache travelled)
            assert int(v0['fver'][d]) != -1 and int(v0['kf_owner'][d]) != -1
        with pytest.raises(_lib.RanSliceError) as ei:
            big.prune(target)
        assert ei.value.code == _lib.RS_ESTATE
        assert _prune_grid(big) == grid
        v = dev.views()
        for e in range(4):
            step = want[e].remove_one()
            assert step['diag_ok'] and (e == 0 or step['slot'] == forced[e])
            assert ((np.diag(want[e].P) <= 0.0).sum() == 1) == (e > 0)
        # first the copies that stand where one removal leaves them, so that a wrong entry is named as the tile and unit it is
        # (a wrong downdate can also keep a copy from stopping: that shows in the sizes and in the message, checked next)
        stopped = [j for j in range(n) if int(v['m'][2 * j]) == SOURCES[int(index[j])] - 1]
        for j in stopped:
            e, d = int(index[j]), 2 * j
            _hold(dev, v, d, want[e], SOURCES[e], 'copy %d of source %d (%d landmarks), its one removal' % (j, e, SOURCES[e]))
            assert int(v['m_last'][d]) == -1 and int(v['kf_owner'][d]) == -1 and int(v['fver'][d]) == -1
            assert int(v['m'][d + 1]) == 0 and int(v['fver'][d + 1]) == int(v0['fver'][d + 1])
        assert len(stopped) == n, 'copies that did not stop after one removal: %s' % sorted(set(range(n)) - set(stopped))[:16]
        assert str(ei.value) == 'libranslice error %d: %s' % (_lib.RS_ESTATE, REFUSED % ('kb_prune', 3 * sets, 0, 3 * sets))
        assert np.array_equal(big.pruned().reshape(-1, 2), np.stack([np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64)], axis=1))
        # the stretches of the round: the plan lists the dictionaries over the target in increasing order
        base = np.concatenate([[0], np.cumsum([dev.line(int(m)) for m in sizes])]).astype(np.int64)
        total = int(base[-1])
        assert total >= 3 * waves
        w = np.arange(waves, dtype=np.int64)
        lo, hi = total * w // waves, total * (w + 1) // waves
        assert (hi - lo >= 3).all()
        slot = np.searchsorted(base, lo, side='right') - 1
        crosses = int((hi > base[slot + 1]).sum())
        inside = int((((lo - base[slot]) & 3) != 0).sum())
        print('work line %d units over %d waves: stretches of %d..%d units, %d cross a dictionary boundary, %d begin inside a tile'
              % (total, waves, (hi - lo).min(), (hi - lo).max(), crosses, inside))
        assert crosses >= 1 and inside >= 1
        # the work counters: one round with work, the units of every dictionary that hold rows
        units = sum(dev.units(int(m)) for m in sizes)
        assert dev.work() == (units, 1), (dev.work(), units)
        big.close()
        src.close()


@pytest.mark.parametrize('grid', [1, 2])
def test_shared_stretches(grid):
    """The same on full storage, where a shared handle's S dictionaries never fill the waves of a co-resident round: the
    downdate's grid is SET to 1 and 2 workgroups (kb_dev_set_prune_grid of the test build), so that the 4 and 8 waves of
    prune_shared_downdate_kernel walk stretches of 45, and of 22 or 23, units of the round's work line.  The shared pair of 321
    and 130 landmarks (6 and 3 blocks: 6 * 6 * 4 + 3 * 3 * 4 = 180 units); dictionary 0 is edited to stop after its first
    removal (_stop_after_one), and shrink(129) takes dictionary 1 to the target in the same single round with work: RS_ESTATE
    with the whole message, both dictionaries where one removal of their mirrors leaves them as bytes -- both stored triangles,
    pages, chains, caches, counters (_hold through _Run.call) --, the work counters at that round's closed form.  Every stretch
    is at least 3 units long, at least one begins inside a tile, at least one crosses from dictionary 0 into dictionary 1."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('RANSLICE_DEV_BUILD', '1')
        h, blob = _base(321, True, dev_build=True)
        dev = _edited(h, blob, lambda dev, v: _stop_after_one(dev, v, 0, 10))
        sizes = [int(m) for m in h.dictionary_sizes()]
        assert sizes == [321, 130]
        assert h.shrink(384) == 0                        # nothing to do: the call only chooses the grid
        chosen = _prune_grid(h)
        run = _Run(h)
        assert run.dev.work() == (0, 0)
        try:
            for bad in (0, -1, chosen + 1):                # (no handle launches more than one co-resident round)
                assert _set_prune_grid(h, bad) == _lib.RS_EINVAL and _prune_grid(h) == chosen
            assert chosen >= grid and _set_prune_grid(h, grid) == _lib.RS_OK and _prune_grid(h) == grid
            logs = run.call(129, 'shared stretches, grid %d' % grid, expect=REFUSED % ('kb_shared_prune', 1, 0, 1), stops={0: 1})
            assert _prune_grid(h) == grid
        finally:
            assert _set_prune_grid(h, chosen) == _lib.RS_OK
        assert logs[0][0]['slot'] == 10 and len(logs[0]) == 1 and len(logs[1]) == 1
        assert (np.diag(run.mirrors[0].P) <= 0.0).sum() == 1, 'the second round must meet exactly one diagonal entry that is not positive'
        assert list(h.dictionary_sizes()) == [320, 129] and list(h.pruned().reshape(-1)) == [1, 1]
        # the stretches of the round with work, from the plan's prefix sums and the grid as wave_share computes them
        base = np.concatenate([[0], np.cumsum([dev.line(m) for m in sizes])]).astype(np.int64)
        total, waves = int(base[-1]), 4 * grid
        assert total == 6 * 6 * 4 + 3 * 3 * 4 == 180
        w = np.arange(waves, dtype=np.int64)
        lo, hi = total * w // waves, total * (w + 1) // waves
        assert (hi - lo >= 3).all()
        slot = np.searchsorted(base, lo, side='right') - 1
        crosses = int((hi > base[slot + 1]).sum())
        inside = int((((lo - base[slot]) & 3) != 0).sum())
        print('work line %d units over %d waves: stretches of %d..%d units, %d cross a dictionary boundary, %d begin inside a tile'
              % (total, waves, (hi - lo).min(), (hi - lo).max(), crosses, inside))
        assert crosses >= 1 and inside >= 1
        # the work counters: one round with work, the units of both dictionaries that hold rows
        assert dev.work() == (sum(dev.units(m) for m in sizes), 1), dev.work()
