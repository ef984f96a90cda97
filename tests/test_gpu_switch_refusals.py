"""The texts and codes of the Projectron++ switches' refusals, whole: kb_set_control_plus, kb_set_control_plus_batch,
kb_set_fit_steps_batch, kb_set_control_plus_wide, kb_set_shared_plus_batch, and beside them kb_set_algorithm, kb_fit and
kb_set_fit_wide / kb_set_fit_wide_plus, which refuse the same handles.  Every case pins kb_last_error's WHOLE string and the return
code; the order of a setter's refusals is pinned by handing a handle that is refused an argument that is refused too.  The
counter readers return zeros while their switch has never been set.

The smallest handles that exist: one replica, capacity 64, reset, no learning step run."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DIMS = [10, 3]
N_PRBS = 9
CAP = 64
PLUS = 1    # KB_ALG_PROJECTRON_PLUS

REF = 'a by-reference handle (kb_deploy_ref)'
FROZEN = 'an inference-only handle (kb_deploy, kb_import_agents)'
SHARED = 'a shared-dictionary handle'
MAXL = " (a multiple of 64, at least 64 and at most the handle's capacity, %d)" % CAP
CTL = ' does not learn through kb_update_control'


@pytest.fixture(scope='module')
def handles():
    """learning, inference-only, by-reference, shared-dictionary"""
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    one = np.full((1, len(DIMS)), 1)
    ag = VecKBRL(1, DIMS, N_PRBS, capacity=CAP, pool_bytes=16 << 20)
    ag.reset(one, one)
    sh = SharedVecKBRL(1, DIMS, N_PRBS, capacity=CAP, pool_bytes=16 << 20)
    sh.reset(one, one)
    hs = {'learning': ag, 'frozen': ag.deploy([0]), 'ref': ag.deploy([0], by_reference=True), 'shared': sh}
    yield hs
    for k in ('frozen', 'ref', 'shared', 'learning'):
        hs[k].close()


def _refused(h, fn, args, code, text):
    rc = getattr(h.L, fn)(h.h, *args)
    err = h.L.kb_last_error(h.h).decode()
    assert (rc, err) == (code, text), (fn, args)


KINDS = (('ref', REF), ('frozen', FROZEN), ('shared', SHARED))


def test_info_is_zero_before_a_switch_is_set(handles):
    for name, h in handles.items():
        for fn in ('kb_control_plus_batch_info', 'kb_control_plus_wide_info', 'kb_fit_steps_batch_info', 'kb_shared_plus_batch_info'):
            w = (C.c_uint64 * 8)(*([7] * 8))
            assert getattr(h.L, fn)(h.h, w) == 0 and [int(v) for v in w] == [0] * 8, (name, fn)
        w = (C.c_uint64 * 4)(*([7] * 4))
        assert h.L.kb_fit_wide_info(h.h, w) == 0 and [int(v) for v in w] == [0] * 4, name
        w, ms = (C.c_uint64 * 4)(*([7] * 4)), (C.c_double * 2)(7.0, 7.0)
        assert h.L.kb_fit_time_ms(h.h, ms, w) == 0 and [int(v) for v in w] == [0] * 4 and list(ms) == [0.0, 0.0], name


@pytest.mark.parametrize('fn,tail', [
    ('kb_set_control_plus_batch', ' (0: the candidates one by one, the default; 2, 4 or 8: that many candidates share one pass over Kinv)'),
    ('kb_set_fit_steps_batch', ' (0: the candidates one by one, the default; 2, 4 or 8: that many candidates of a row share one pass over Kinv)')])
def test_width_setters(handles, fn, tail):
    from ranslice import _lib
    through = CTL if fn == 'kb_set_control_plus_batch' else ' does not learn through kb_fit_steps'
    ag = handles['learning']
    for w in (1, 3, 5, 6, 7, 9, 16, -2):
        _refused(ag, fn, (w, 64), _lib.RS_EINVAL, '%s: width = %d%s' % (fn, w, tail))
    for mx in (0, 63, 32, 100, 128, -64):
        _refused(ag, fn, (8, mx), _lib.RS_EINVAL, '%s: max_landmarks = %d%s' % (fn, mx, MAXL))
    _refused(ag, fn, (3, 100), _lib.RS_EINVAL, '%s: width = 3%s' % (fn, tail))             # the width first
    for kind, what in KINDS:
        h = handles[kind]
        _refused(h, fn, (8, 64), _lib.RS_ESTATE, '%s: %s%s' % (fn, what, through))
        _refused(h, fn, (0, 0), _lib.RS_ESTATE, '%s: %s%s' % (fn, what, through))          # turning it off is refused too
        _refused(h, fn, (3, 64), _lib.RS_EINVAL, '%s: width = 3%s' % (fn, tail))           # the arguments before the handle
        _refused(h, fn, (8, 100), _lib.RS_EINVAL, '%s: max_landmarks = 100%s' % (fn, MAXL))


def test_control_plus_wide(handles):
    from ranslice import _lib
    fn = 'kb_set_control_plus_wide'
    ag = handles['learning']
    for mx in (0, 63, 32, 100, 128, -64):
        _refused(ag, fn, (2, mx, 4), _lib.RS_EINVAL, '%s: max_landmarks = %d%s' % (fn, mx, MAXL))
    mins = ' (0 turns the rounds off, the default; else 2 .. max_landmarks = 64: a single landmark\'s float32 regime stays on the batch kernel\'s row)'
    for mn in (1, -2, 65):
        _refused(ag, fn, (mn, 64, 4), _lib.RS_EINVAL, '%s: min_landmarks = %d%s' % (fn, mn, mins))
    for r in (0, 257, -1):
        _refused(ag, fn, (2, 64, r), _lib.RS_EINVAL, '%s: rounds = %d (1 .. 256 rounds enqueued per update phase)' % (fn, r))
    _refused(ag, fn, (1, 100, 0), _lib.RS_EINVAL, '%s: max_landmarks = 100%s' % (fn, MAXL))    # max, then min, then rounds
    _refused(ag, fn, (1, 64, 0), _lib.RS_EINVAL, '%s: min_landmarks = 1%s' % (fn, mins))
    for kind, what in KINDS:
        h = handles[kind]
        _refused(h, fn, (2, 64, 4), _lib.RS_ESTATE, '%s: %s%s' % (fn, what, CTL))
        _refused(h, fn, (0, 0, 0), _lib.RS_ESTATE, '%s: %s%s' % (fn, what, CTL))
        _refused(h, fn, (2, 64, 0), _lib.RS_EINVAL, '%s: rounds = 0 (1 .. 256 rounds enqueued per update phase)' % fn)


def test_shared_plus_batch(handles):
    from ranslice import _lib
    fn = 'kb_set_shared_plus_batch'
    sh = handles['shared']
    mins = " (0 turns the segments off, the default; else 2 .. the handle's capacity, %d: a single landmark's float32 regime stays one by one)" % CAP
    segs = ' (0 .. 16 segment rounds enqueued per apply; the finishing launch takes what they leave)'
    for mn in (1, -1, 65):
        _refused(sh, fn, (mn, 4), _lib.RS_EINVAL, '%s: min_landmarks = %d%s' % (fn, mn, mins))
    for sg in (-1, 17):
        _refused(sh, fn, (2, sg), _lib.RS_EINVAL, '%s: segments = %d%s' % (fn, sg, segs))
    _refused(sh, fn, (0, 17), _lib.RS_EINVAL, '%s: segments = 17%s' % (fn, segs))
    _refused(sh, fn, (1, 17), _lib.RS_EINVAL, '%s: min_landmarks = 1%s' % (fn, mins))          # min_landmarks first
    for kind in ('learning', 'frozen', 'ref'):
        h = handles[kind]
        _refused(h, fn, (2, 4), _lib.RS_ESTATE, '%s: not a shared-dictionary handle' % fn)
        _refused(h, fn, (0, 0), _lib.RS_ESTATE, '%s: not a shared-dictionary handle' % fn)
        _refused(h, fn, (2, 17), _lib.RS_EINVAL, '%s: segments = 17%s' % (fn, segs))


def test_control_plus_algorithm_fit_wide_and_fit(handles):
    from ranslice import _lib
    ag = handles['learning']
    on_cp = ' (0: the control loop refuses Projectron++ mode, the default; 1: it learns by the margin rule)'
    on_fw = ' (0: Projectron++ keeps the narrow path, the default; 1: the rounds teach it too)'
    for on in (2, -1):
        _refused(ag, 'kb_set_control_plus', (on,), _lib.RS_EINVAL, 'kb_set_control_plus: on = %d%s' % (on, on_cp))
        _refused(ag, 'kb_set_fit_wide_plus', (on,), _lib.RS_EINVAL, 'kb_set_fit_wide_plus: on = %d%s' % (on, on_fw))
    for alg in (2, -1, 7):
        _refused(ag, 'kb_set_algorithm', (alg,), _lib.RS_EINVAL,
                 'kb_set_algorithm: %d names no algorithm (KB_ALG_PROJECTRON, KB_ALG_PROJECTRON_PLUS)' % alg)
    fit_args = (None, 0, None, None, None, 0, None, None, None, None, None)
    cannot = {'ref': ': a by-reference handle (kb_deploy_ref) shares read-only dictionaries: it cannot learn',
              'frozen': ': an inference-only handle (kb_deploy, kb_import_agents) cannot learn: it holds no Kinv',
              'shared': ': shared-dictionary handles are not supported: several learners map to one dictionary'}
    for kind, what in KINDS:
        h = handles[kind]
        for on in (0, 1):
            _refused(h, 'kb_set_control_plus', (on,), _lib.RS_ESTATE, 'kb_set_control_plus: %s%s' % (what, CTL))
            _refused(h, 'kb_set_fit_wide_plus', (on,), _lib.RS_ESTATE, 'kb_set_fit_wide_plus: %s does not learn through kb_fit' % what)
        _refused(h, 'kb_set_control_plus', (2,), _lib.RS_EINVAL, 'kb_set_control_plus: on = 2%s' % on_cp)
        _refused(h, 'kb_set_fit_wide', (2, 0), _lib.RS_ESTATE, 'kb_set_fit_wide: %s does not learn through kb_fit' % what)
        _refused(h, 'kb_set_fit_wide', (0, 0), _lib.RS_ESTATE, 'kb_set_fit_wide: %s does not learn through kb_fit' % what)
        _refused(h, 'kb_set_algorithm', (PLUS,), _lib.RS_ESTATE,
                 'kb_set_algorithm: %s does not learn through kb_update / kb_fit: Projectron++ has nothing to act on' % what)
        _refused(h, 'kb_set_algorithm', (7,), _lib.RS_EINVAL, 'kb_set_algorithm: 7 names no algorithm (KB_ALG_PROJECTRON, KB_ALG_PROJECTRON_PLUS)')
        assert h.L.kb_set_algorithm(h.h, 0) == 0                                               # Projectron is what such a handle is in
        _refused(h, 'kb_fit', fit_args, _lib.RS_ESTATE, 'kb_fit' + cannot[kind])
    # the learning handle takes all of them, and gives the scratch back
    assert ag.L.kb_set_algorithm(ag.h, PLUS) == 0 and ag.L.kb_set_control_plus(ag.h, 1) == 0
    assert ag.L.kb_set_control_plus_batch(ag.h, 8, 64) == 0 and ag.L.kb_set_control_plus_wide(ag.h, 2, 64, 4) == 0
    assert ag.L.kb_set_fit_steps_batch(ag.h, 4, 64) == 0
    T = len(DIMS)
    assert ag.control_plus_batch == (8, 64, 128 + T * 2 * 8 * 64 * 8) and ag.fit_steps_batch == (4, 64, 128 + T * 2 * 4 * 64 * 8)
    assert ag.control_plus_wide == (2, 64, 4, 128 + T * 256 + 2 * (T + 1) * 8 + 8 * ((T + 1) // 2) + T * 2 * 8 * 64 * 8)
    assert ag.control_plus_batch_work() == [0] * 8 and ag.control_plus_wide_work() == [0] * 8 and ag.fit_steps_batch_work() == [0] * 8
    assert ag.L.kb_set_control_plus_wide(ag.h, 0, 0, 0) == 0 and ag.L.kb_set_control_plus_batch(ag.h, 0, 0) == 0
    assert ag.L.kb_set_fit_steps_batch(ag.h, 0, 0) == 0
    assert ag.control_plus_batch == (0, 0, 0) and ag.fit_steps_batch == (0, 0, 0) and ag.control_plus_wide == (0, 0, 0, 0)
    assert ag.L.kb_set_control_plus(ag.h, 0) == 0 and ag.L.kb_set_algorithm(ag.h, 0) == 0
