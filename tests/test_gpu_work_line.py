"""The work-line helpers of csrc/kb_kbrl.hip ON THE DEVICE, by themselves: kb_dev_work_line of the test build (csrc/kb_probe.hip)
runs walk_stretch and block_scan1024 on lines this file supplies.  Every kernel that spreads work by cost -- the repair rounds,
kb_prune's downdate, kb_fit's chip-wide rounds -- lays its work out with that scan and hands it to its waves with that walker, so
a unit nobody takes, or two waves take, is a wrong Kinv there.  All integer: every comparison is exact.

The walker: every unit of the line is hit exactly once, and by the slot that owns it, at 8 workgroups (32 waves) and at one.
The scan: the inclusive sums of the one-value and the two-value form equal numpy.cumsum, across passes of 1,024 with a carry.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _probe(op, inp, count, grid, out0, out1):
    from ranslice import _lib
    L = _lib.load(dev=True)
    L.kb_dev_work_line.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.kb_dev_work_line.restype = C.c_int
    inp = np.ascontiguousarray(inp, dtype=np.int64)
    rc = L.kb_dev_work_line(0, op, inp.ctypes.data_as(C.POINTER(C.c_int64)), count, grid, out0.ctypes.data_as(C.c_void_p),
                            out1.ctypes.data_as(C.c_void_p))
    assert rc == 0, 'kb_dev_work_line(op %d) returned %d' % (op, rc)


WIDTHS = {
    'one unit: 31 of 32 waves get nothing': [1],
    'empty slots first, inside and last': [0, 3, 0, 0, 7, 0],
    'one slot cut by many waves': [1000, 1],
    'no work at all': [0, 0, 0, 0, 0],
    '1,025 slots of widths 0..5': np.random.default_rng(20251).integers(0, 6, size=1025).tolist(),
}


@pytest.mark.parametrize('grid', [8, 1])
@pytest.mark.parametrize('case', list(WIDTHS))
def test_walker_hands_out_every_unit_once(case, grid):
    widths = np.asarray(WIDTHS[case], dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(widths)])
    total = int(base[-1])
    hits = np.full(total + 1, 7, dtype=np.int32)  # (the probe returns one entry past the line, which nobody may touch)
    owner = np.full(total + 1, 7, dtype=np.int32)
    _probe(0, base, len(widths), grid, hits, owner)
    want = np.repeat(np.arange(len(widths), dtype=np.int32), widths)
    assert (hits[:total] == 1).all(), 'units hit other than once: %s' % {int(u): int(hits[u]) for u in np.flatnonzero(hits[:total] != 1)[:8]}
    assert (owner[:total] == want).all(), 'units handed out under the wrong slot: first at %d' % int(np.argmin(owner[:total] == want))
    assert hits[total] == 0 and owner[total] == -1, 'a unit past the end of the line was handed out'


@pytest.mark.parametrize('count', [1, 1023, 1024, 1025, 2049])
def test_scans_equal_cumsum(count):
    vals = np.random.default_rng(count).integers(0, (1 << 40) + 1, size=(2, count), dtype=np.int64)
    one = np.zeros(count, dtype=np.int64)
    two = np.zeros((2, count), dtype=np.int64)
    _probe(1, vals, count, 1, one, two)
    ref = np.cumsum(vals, axis=1)
    assert (one == ref[0]).all(), 'one-value scan: first difference at %d' % int(np.argmin(one == ref[0]))
    assert (two == ref).all(), 'two-value scan: first difference at %s' % (np.argwhere(two != ref)[:1].tolist(),)
