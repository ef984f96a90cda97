"""ProjectronPlus.update ON THE DEVICE, stage by stage (csrc/kb_kbrl.hip: predict_column, apply_update_plus, margin_update), against
tests/update_mirror.py's step_plus and against exact arithmetic (exact_plus, plus_bounds).

  (a) one margin step per case of the rule -- branch 0, branch 4, and branch 3 with each of the three terms of alpha winning -- on a
      ladder of dictionary sizes in ONE handle, through kb_predict / kb_update: f, K_f, d*, delta and the coefficients after equal
      the mirror's as BITS (the mirror is fed what the device held before the step), branch, winning term and size exactly, Kinv
      and the landmarks unchanged bytes; f and the new coefficients keep the derived forward bounds against exact arithmetic.
  (b) the float32 regime of one landmark with a coefficient other than +-1, built by hand: all five cases, and the two exact ties
      (loss / norm == 1.0, slack == 0.0) that alone can show the order of the three comparisons and the sign of the slack test.
  (c) the same steps of (a), in their order, through kb_fit (fit_plus_kernel) in the handle's other replicas and through the chip-wide
      rounds (kb_set_fit_wide(2) with kb_set_fit_wide_plus) in a second handle grown identically: equal bytes before, f / delta / branch
      as returned, coefficients and Kinv as bytes after, and the K_f and d* rows.  Which rows a path leaves: every path writes the
      K_f row on every sample (predict_column; the rounds' decide kernel for the sample it stops at and for a chunk's last); the
      d* row is written by every sample of branches 1-4 and left alone by branch 0, so it is compared on branches 3 and 4 only.
  (d) the mirror walks ALONE over whole stretches of the reference's recording G18 that ONE kb_fit call learns: every sample's f
      and delta as bits, branch and size, the dictionary at the end as bytes, and the K_f / d* rows the last samples left.

kb_fit_steps and control_plus_kernel run the same fit_rule<PROJECTRON_PLUS>; tests/test_gpu_fit_steps.py and
tests/test_gpu_control_plus.py hold them to kb_fit's bytes row by row, so they are left out here.

Run with -s for the cases found per size and the largest error / bound ratios (DESIGN.md §8i quotes them).
"""
import os

import numpy as np
import pytest

import update_mirror as um
from test_gpu_kbrl import _fast_growing_samples
from test_gpu_update_chain import _prefix_lengths, _stream3, bits, dev_agent, same, update_rows

pytestmark = pytest.mark.gpu

GAMMA, ETA, N_PRBS = 1.0, 0.1, 200
PLUS = 'projectron_plus'
L10, L3 = um.PLUS_LADDER10, um.PLUS_LADDER3


def _tag(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, 'g18_projectron_plus.npz'))
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + '_')}


def _device_step(ag, e, s, x, y, m):
    """kb_predict / kb_update of learner (e, s) -> what the device held before, returned, and left"""
    b = ag.learner(e, s)
    y_pred, f = ag.predict(e, s, x)
    br, delta = ag.update(e, s, x, y)
    a = ag.learner(e, s)
    kf, ds, parts = update_rows(ag, e, s, m)
    return dict(before=b, y_pred=y_pred, f=f, branch=br, delta=delta, after=a, kf=kf, ds=ds, parts=parts, x=x, y=y)


def _check_step(rec, kinv, tag, want=None, kinv_ld=None):
    """one recorded device step against step_plus on what the device held, and against exact arithmetic -> (the mirror's case,
    dict of error / bound ratios)"""
    b, a, x, y = rec['before'], rec['after'], rec['x'], rec['y']
    m = b['m']
    mir = um.step_plus(kinv, b['coeff'], b['landmarks'], x, y, GAMMA, ETA)
    case = {0: 'branch0', 4: 'branch4', 3: mir['won']}.get(mir['branch'])
    tag = tag + ('m %d' % m, case)
    if want is not None:
        assert case == want, tag + ('the mirror names another case than the preselection', mir['branch'], mir['terms'], mir['slack'])
    assert bits(np.float64(rec['f'])) == bits(np.float64(mir['f'])), tag + ('f', rec['f'], mir['f'])
    assert rec['y_pred'] == (1 if mir['f'] > 0 else -1), tag
    kf, ds, parts = rec['kf'], rec['ds'], rec['parts']
    assert same(kf, mir['column']), tag + ('K_f', int((bits(kf) != bits(mir['column'])).sum()))
    if mir['branch'] != 0 and not same(ds, mir['dstar']):     # name the stage: the tiles' partial sums, or the combine
        live = lambda blk: min(64, m - 64 * blk)
        bad = [t for t in mir['dpart'] if not same(parts[t][:live(t[1])], mir['dpart'][t][:live(t[1])])
               or (t in mir['tpart'] and not same(parts[t][64:64 + live(t[0])], mir['tpart'][t][:live(t[0])]))]
        raise AssertionError(tag + ('d*: %d of %d outputs differ' % (int((bits(ds) != bits(mir['dstar'])).sum()), m),
                                    'partial sums differ in tiles %s' % bad[:6] if bad else 'every partial sum equal: the combine'))
    assert rec['branch'] == mir['branch'], tag + (rec['branch'], mir['branch'], mir['slack'])
    assert bits(np.float64(rec['delta'])) == bits(np.float64(mir['delta'])), tag + ('delta', rec['delta'], mir['delta'])
    assert a['m'] == mir['m'] == m, tag
    assert same(a['landmarks'], b['landmarks']), tag + ('landmarks',)
    assert same(a['coeff'], mir['coeff']), tag + ('coefficients', int((bits(a['coeff']) != bits(mir['coeff'])).sum()))
    if mir['branch'] != 3:
        assert same(a['coeff'], b['coeff']), tag + ('coefficients moved',)
    # exact arithmetic on the device's own doubles
    ex = um.exact_plus(kinv if kinv_ld is None else kinv_ld, kf, b['coeff'], y, ETA)
    bd = um.plus_bounds(ex, m, ETA)
    rt = um.plus_ratios(dict(f=rec['f'], coeff=a['coeff'] if mir['branch'] == 3 else None, dstar=ds if mir['branch'] != 0 else None),
                        ex, bd)
    assert all(v <= 1.0 for v in rt.values()), tag + ('error / bound', rt)
    return case, rt, ex, bd


# ------------------------------------------------------------------ (a), (c) the ladder, on three paths
def _grow(h, learners, cut, streams, n10):
    h.fit(learners, [streams[s][0][:cut[s][e % n10]] for e, s in learners], [streams[s][1][:cut[s][e % n10]] for e, s in learners])


@pytest.fixture(scope='module')
def grown():
    """23 learners of ten state variables at 1 .. 641 landmarks and 15 of three at 1 .. 193, grown in Projectron mode with kb_fit
    from prefixes of one stream per kind, and the same ladder in the handle's other replicas (kb_fit's twins); then the handle
    switches to Projectron++.  -> dict(ag, n10, learners [(e, s)], sizes, cut, streams, full: per learner what it and its twin hold,
    Kinv included)"""
    n10, n3 = len(L10), len(L3)
    with pytest.MonkeyPatch.context() as mp:
        ag = dev_agent(mp, 2 * n10 + 1, [10, 3], N_PRBS, capacity=1024, gamma=GAMMA, eta=ETA)
    try:
        zero = np.zeros((ag.n_envs, 2), dtype=np.int32)
        ag.reset(zero, zero)
        streams = [_fast_growing_samples(4600), _stream3(3000)]
        pilot = ag.n_envs - 1       # one learner per kind takes the whole stream and says where every size is reached
        r = ag.fit([(pilot, 0), (pilot, 1)], [streams[0][0], streams[1][0]], [streams[0][1], streams[1][1]])
        cut = [_prefix_lengths(r['m'][0], L10), _prefix_lengths(r['m'][1], L3)]
        first = [(e, s) for s, n in ((0, n10), (1, n3)) for e in range(n)]
        sizes = [(L10, L3)[s][e] for e, s in first]
        _grow(ag, first + [(e + n10, s) for e, s in first], cut, streams, n10)
        ag.set_algorithm(PLUS)
        full = [[ag.learner(e, s, with_kinv=True), ag.learner(e + n10, s, with_kinv=True)] for e, s in first]
        yield dict(ag=ag, n10=n10, learners=first, sizes=sizes, cut=cut, streams=streams, full=full)
    finally:
        ag.close()


def test_ladder_is_grown_to_the_same_bytes_twice(grown):
    """every size of the ladder is reached, and the learner and its twin in the same handle hold the same landmarks, coefficients
    and Kinv before the first margin step (the second handle's: test_ladder_margin_steps_through_kb_fit_and_the_rounds_...)"""
    ag = grown['ag']
    assert ag.algorithm == PLUS and ag.fit_wide == (0, 0)
    for (e, s), m, full in zip(grown['learners'], grown['sizes'], grown['full']):
        assert [L['m'] for L in full] == [m] * 2, (s, m, [L['m'] for L in full])
        for k in ('landmarks', 'coeff', 'kinv'):
            assert same(full[0][k], full[1][k]), ('the twin differs before the steps', k, s, m)
        assert same(full[0]['kinv'], full[0]['kinv'].T)


@pytest.fixture(scope='module')
def ladder(grown):
    """The device side of (a), run once.  Per learner and case, in the order of update_mirror.CASES, a sample is preselected from
    the coefficients the device holds NOW (update_mirror.PlusInputs) and taken through kb_predict / kb_update.
    -> [(dims, m, Kinv, [per case: dict(case, step)], the learner's PlusInputs)]"""
    ag = grown['ag']
    out = []
    for (e, s), m, full in zip(grown['learners'], grown['sizes'], grown['full']):
        inp = um.PlusInputs(full[0]['kinv'], full[0]['landmarks'], GAMMA, ETA, N_PRBS)
        steps = []
        for case in um.CASES:
            p = inp.pick(ag.learner(e, s)['coeff'], case)
            if p is not None:
                steps.append(dict(case=case, step=_device_step(ag, e, s, p[0], p[1], m)))
        end = ag.learner(e, s, with_kinv=True)
        assert same(end['kinv'], full[0]['kinv']) and same(end['landmarks'], full[0]['landmarks']) and end['m'] == m, \
            ('Kinv or the landmarks changed under the margin rule', s, m)
        out.append(((10, 3)[s], m, full[0]['kinv'], steps, inp))
    return out


@pytest.fixture(scope='module')
def twins(grown, ladder):
    """The device side of (c): a second handle grown as the first was, switched to Projectron++ with the rounds on from two
    landmarks; then every learner's steps of (a), in their order, by its twin in the first handle through kb_fit and by its twin in
    the second through the rounds.  -> per learner [per step: dict(fit, wide)], aligned with `ladder`"""
    ag, n10 = grown['ag'], grown['n10']
    with pytest.MonkeyPatch.context() as mp:
        wd = dev_agent(mp, n10, [10, 3], N_PRBS, capacity=1024, gamma=GAMMA, eta=ETA)
    try:
        zero = np.zeros((wd.n_envs, 2), dtype=np.int32)
        wd.reset(zero, zero)
        _grow(wd, grown['learners'], grown['cut'], grown['streams'], n10)
        wd.set_algorithm(PLUS)
        wd.set_fit_wide(2, 0)
        wd.set_fit_wide_plus(True)
        assert wd.algorithm == PLUS and wd.fit_wide == (2, 0) and wd.fit_wide_plus is True
        out = []
        for (e, s), m, full, (_, _, _, steps, _) in zip(grown['learners'], grown['sizes'], grown['full'], ladder):
            w0 = wd.learner(e, s, with_kinv=True)
            assert w0['m'] == m and all(same(w0[k], full[0][k]) for k in ('landmarks', 'coeff', 'kinv')), \
                ('the second handle differs before the steps', s, m)
            recs = []
            for st in steps:
                x, y = st['step']['x'], st['step']['y']
                rec = dict(fit=dict(before=ag.learner(e + n10, s), out=ag.fit([(e + n10, s)], [x[None]], [[y]]),
                                    after=ag.learner(e + n10, s), rows=update_rows(ag, e + n10, s, m, False)), wide=None)
                if m >= 2:
                    rec['wide'] = dict(before=wd.learner(e, s), out=wd.fit([(e, s)], [x[None]], [[y]]), after=wd.learner(e, s),
                                       rows=update_rows(wd, e, s, m, False), info=wd.fit_wide_info())
                recs.append(rec)
            for name, L in (('kb_fit', ag.learner(e + n10, s, with_kinv=True)), ('rounds', wd.learner(e, s, with_kinv=True))):
                assert same(L['kinv'], full[0]['kinv']) and same(L['landmarks'], full[0]['landmarks']) and L['m'] == m, \
                    ('Kinv or the landmarks changed under the margin rule', name, s, m)
            out.append(recs)
        yield out
    finally:
        wd.close()


def test_ladder_margin_steps_of_kb_update_give_the_mirrors_bits(ladder):
    """(a).  No case is dropped silently: at every size from 63 up all five cases are found and run, at 2 .. 9 at least branch 4 and
    branch 3 by loss / norm and by 2 slack / norm (update_mirror.cases_required).  The preselection's clearance of 1e-6 is more
    than a thousand times the derived bound of every quantity it decides on from two landmarks on, and above the float32 bounds
    while one landmark is held."""
    worst, table = {}, []
    for dims, m, kinv, steps, inp in ladder:
        ran, row = [], {}
        kinv_ld = kinv.astype(np.longdouble)
        for st in steps:
            case, rt, ex, bd = _check_step(st['step'], kinv, ('dims %d' % dims,), want=st['case'], kinv_ld=kinv_ld)
            ran.append(case)
            decides = [bd['f']] + ([bd['slack']] if case != 'branch0' else []) + \
                      ([bd['terms'][0], bd['terms'][2]] if case in um.TERMS else [])
            # (one landmark: f, margin and loss are float32, their bounds 2^-24 of their size -- the clearance exceeds them, not 1000-fold)
            assert (1000.0 if m >= 2 else 1.0) * max(decides) < um.CLEARANCE, ('dims %d' % dims, m, case, 'the clearance', decides)
            if case != 'branch0':
                assert st['step']['branch'] == ex['branch'] and (case not in um.TERMS or (bd['won_clear'] and ex['won'] == case)), \
                    ('dims %d' % dims, m, case, 'exact arithmetic names another case')
            for k, v in rt.items():
                row[k] = max(row.get(k, 0.0), v)
                worst[k] = max(worst.get(k, 0.0), v)
        if not set(um.cases_required(m)) <= set(ran):
            raise AssertionError(('dims %d' % dims, m, 'cases not found', ran, inp.counts(steps[-1]['step']['after']['coeff'])))
        table.append('dims %2d m %3d: ran %-36s error / bound %s'
                     % (dims, m, ','.join(ran), ' '.join('%s %.3g' % kv for kv in sorted(row.items()))))
    print('\n'.join(table))
    print('ladder: largest error / bound: %s' % ' '.join('%s %.3g' % kv for kv in sorted(worst.items())))


def test_ladder_margin_steps_through_kb_fit_and_the_rounds_leave_the_same_bytes(ladder, twins):
    """(c).  The twin of every step of (a) through fit_plus_kernel, and from two landmarks on through the chip-wide rounds (the
    info counts the sample and, off branch 0, its mat-vec: it did go wide)."""
    n = dict(fit=0, wide=0)
    for (dims, m, kinv, steps, _), recs in zip(ladder, twins):
        for st, rec in zip(steps, recs):
            ref = st['step']
            for path in ('fit', 'wide'):
                tw = rec[path]
                if tw is None:
                    assert path == 'wide' and m < 2
                    continue
                tag = ('dims %d' % dims, 'm %d' % m, st['case'], path)
                for k in ('landmarks', 'coeff'):
                    assert same(tw['before'][k], ref['before'][k]), tag + ('differs before the step', k)
                o = tw['out']
                assert int(o['y_pred'][0][0]) == ref['y_pred'] and int(o['branch'][0][0]) == ref['branch'] and int(o['m'][0][0]) == m, tag
                assert bits(o['f'][0])[0] == bits(np.float64(ref['f'])) and bits(o['delta'][0])[0] == bits(np.float64(ref['delta'])), \
                    tag + ('f or delta', o['f'][0][0], ref['f'], o['delta'][0][0], ref['delta'])
                assert tw['after']['m'] == m and same(tw['after']['coeff'], ref['after']['coeff']), tag + ('coefficients after',)
                assert same(tw['rows'][0], ref['kf']), tag + ('the K_f row',)
                if ref['branch'] != 0:
                    assert same(tw['rows'][1], ref['ds']), tag + ('the d* row',)
                if path == 'wide':
                    assert (tw['info']['samples'], tw['info']['matvecs']) == (1, int(ref['branch'] != 0)), tag + (tw['info'],)
                n[path] += 1
    print('twin steps: kb_fit %d, rounds %d' % (n['fit'], n['wide']))
    assert n['fit'] >= 150 and n['wide'] >= 140


# ------------------------------------------------------------------ (b) one landmark, float32
def test_one_landmark_with_a_small_coefficient_meets_every_case_in_float32(monkeypatch):
    """x0 inserted with y = +1, a point 0.05 away on every state coordinate projected with y = -1 (delta 0.049: the coefficient
    becomes about 0.025, a float32), then ONE sample with y = +1 per learner: kernel values to x0 of about 1, 0.98, 0.955 and 0.94 and
    the two exact ties of update_mirror.one_landmark_inputs; x0 itself against a coefficient of 1 has margin == 1.0 exactly.  The
    mirror's stages say which case each is; all five are met, loss is the float32 one and the coefficient is stored as float32."""
    inp = um.one_landmark_inputs(GAMMA, ETA)
    x0, points = inp['x0'], inp['points']
    assert all(x is not None for _, _, x in points)
    ag = dev_agent(monkeypatch, len(points) + 1, [10], N_PRBS, capacity=64, gamma=GAMMA, eta=ETA, algorithm=PLUS)
    try:
        zero = np.zeros((ag.n_envs, 1), dtype=np.int32)
        ag.reset(zero, zero)
        one = np.ones((1, 1))
        met, worst, other_loss = {}, {}, 0
        for e, (name, near, x) in enumerate(points + [('x0', None, x0)]):
            ag.predict(e, 0, x0)
            assert ag.update(e, 0, x0, 1)[0] == 2
            if near is not None:
                ag.predict(e, 0, near)
                br, delta = ag.update(e, 0, near, -1)
                assert br == 1 and (0.04 < delta <= ETA if name.startswith('tie') else abs(delta - 0.049) < 1e-3), (name, br, delta)
            L = ag.learner(e, 0, with_kinv=True)
            assert L['m'] == 1 and same(L['kinv'], one)
            rec = _device_step(ag, e, 0, x, 1, 1)
            case, rt, ex, bd = _check_step(rec, one, (name,))
            mir = um.step_plus(one, rec['before']['coeff'], rec['before']['landmarks'], x, 1, GAMMA, ETA)
            met.setdefault(case, []).append(name)
            if name == 'x0':
                assert mir['margin'] == 1.0 and case == 'branch0'
            else:
                c = rec['before']['coeff'][0]
                assert 0.02 < c < 0.05 and c == np.float32(c)
                assert mir['loss'] == np.float32(mir['loss'])
                other_loss += mir['loss'] != 1.0 - mir['margin']       # (the float64 loss is another number)
                assert rec['after']['coeff'][0] == np.float32(rec['after']['coeff'][0])
            if name == 'tie_alpha':
                assert mir['terms'][0] == 1.0 and case == 'loss' and mir['alpha'] == 1.0
            if name == 'tie_slack':
                assert mir['slack'] == 0.0 and case == 'branch4'
            L2 = ag.learner(e, 0, with_kinv=True)
            assert same(L2['kinv'], one) and same(L2['landmarks'], L['landmarks'])
            for k, v in rt.items():
                worst[k] = max(worst.get(k, 0.0), v)
        print('one landmark: %s; largest error / bound: %s' % (met, ' '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
        assert set(met) == set(um.CASES) and other_loss >= 3, (met, other_loss)
        assert met['loss'][0] == 'k1.0' and 'k0.98' in met['one'] and 'k0.955' in met['slack'] and 'k0.94' in met['branch4']
    finally:
        ag.close()


# ------------------------------------------------------------------ (d) the mirror walks alone
STRETCHES = [      # (tag, learner, first sample, end, branch counts 0 .. 4 the stretch is chosen for, sizes it passes)
    ('d4', (0, 1), 0, 1200, None, (1, 2)),
    ('rev', (0, 0), 338, 438, [21, 4, 13, 8, 54], (64, 65)),
    ('rev', (1, 0), 730, 760, [7, 0, 6, 4, 13], (128, 129)),
]


def test_the_mirror_walks_alone_through_whole_fit_calls(golden_dir, monkeypatch):
    """Each stretch is ONE kb_fit call behind a kb_fit of the samples before it; step_plus runs from the state read at its start
    with nothing re-read in between, so the state it carries -- coefficients, Kinv, landmarks, and the K_f and d* rows a sample
    leaves behind for the next ones (a branch-4 sample writes d* and nothing else) -- is what the device carries.  A sample with
    f == 0 on a populated dictionary draws its sign on the device and is a mistake either way: y_pred is compared where f != 0."""
    ag = dev_agent(monkeypatch, 2, [10, 3], N_PRBS, capacity=1024, gamma=GAMMA, eta=ETA, algorithm=PLUS)
    try:
        zero = np.zeros((2, 2), dtype=np.int32)
        ag.reset(zero, zero)
        for tag, (e, s), i0, i1, counts, passes in STRETCHES:
            g = _tag(golden_dir, tag)
            x, y = g['x'], g['y'].astype(np.int64)
            if i0:
                ag.fit([(e, s)], [x[:i0]], [y[:i0]])
            L = ag.learner(e, s, with_kinv=True)
            m0 = L['m']
            kf_row, ds_row = np.zeros(1024), np.zeros(1024)
            kf_known, ds_known = np.zeros(1024, dtype=bool), np.zeros(1024, dtype=bool)
            if m0:
                kf_row[:m0], ds_row[:m0], _ = update_rows(ag, e, s, m0, False)
                kf_known[:m0] = ds_known[:m0] = True
            r = ag.fit([(e, s)], [x[i0:i1]], [y[i0:i1]])
            state = (L['kinv'] if m0 else np.zeros((0, 0)), L['coeff'], L['landmarks'])
            br = []
            for t in range(i1 - i0):
                st = um.step_plus(*state, x[i0 + t], int(y[i0 + t]), GAMMA, ETA)
                at = (tag, 'sample %d' % (i0 + t), 'm %d' % len(state[1]))
                assert bits(r['f'][0][t:t + 1])[0] == bits(np.float64(st['f'])), at + ('f', r['f'][0][t], st['f'])
                assert int(r['branch'][0][t]) == st['branch'] and int(r['m'][0][t]) == st['m'], at + (r['branch'][0][t], st['branch'])
                assert bits(r['delta'][0][t:t + 1])[0] == bits(np.float64(st['delta'])), at + ('delta', r['delta'][0][t], st['delta'])
                if st['f'] != 0.0:
                    assert int(r['y_pred'][0][t]) == (1 if st['f'] > 0 else -1), at
                mb = len(state[1])
                kf_row[:mb], kf_known[:mb] = st['column'], True
                if st['branch'] != 0:
                    ds_row[:mb], ds_known[:mb] = st['dstar'], True
                if st['branch'] == 2:
                    ds_row[mb], ds_known[mb] = -1.0, True
                br.append(st['branch'])
                state = (st['kinv'], st['coeff'], st['landmarks'])
            assert np.array_equal(br, g['branch'][i0:i1])
            if counts is not None:
                assert np.bincount(br, minlength=5).tolist() == counts, (tag, i0, np.bincount(br, minlength=5))
            sizes = np.concatenate([[m0], r['m'][0]])
            assert all(p in sizes for p in passes), (tag, i0, sizes[0], sizes[-1])
            end = ag.learner(e, s, with_kinv=True)
            assert end['m'] == len(state[1])
            for k, v in zip(('kinv', 'coeff', 'landmarks'), state):
                assert same(end[k], v), (tag, i0, 'the dictionary at the end', k, int((bits(end[k]) != bits(v)).sum()))
            kf, ds, _ = update_rows(ag, e, s, end['m'], False)
            kk, dk = kf_known[:end['m']], ds_known[:end['m']]
            assert same(kf[kk], kf_row[:end['m']][kk]) and same(ds[dk], ds_row[:end['m']][dk]), (tag, i0, 'the K_f / d* rows at the end')
            print('%s %d .. %d: %d -> %d landmarks, branches 0-4 %s' % (tag, i0, i1 - 1, m0, end['m'], np.bincount(br, minlength=5).tolist()))
    finally:
        ag.close()
