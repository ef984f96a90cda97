"""Agent files on the host (no GPU): the format round trip of ranslice.agent_file, kb_agents_info of the product library on good
and on damaged blobs (it makes no device call), and the yardstick of the device test -- tests/agent_restatement.py held to what
the reference itself recorded in the four KBRL fixtures."""
import struct
import types

import numpy as np
import pytest

import agent_restatement as ar
from ranslice import _lib, agent_file as af

SIZES = [0, 1, 2, 63, 64, 65, 513]
DIMS = [10, 3]
N_PRBS = 50


def make_agents(n_agents, seed=1, sizes=SIZES, dims=DIMS, n_prbs=N_PRBS):
    """agents whose dictionaries walk through `sizes` (every size with dims 10 and with dims 3 once n_agents * 2 >= 2 * 7)"""
    rng = np.random.default_rng(seed)
    S, agents, k = len(dims), [], 0
    for j in range(n_agents):
        lms, cos = [], []
        for s in range(S):
            m = sizes[(k + (len(sizes) // 2) * s) % len(sizes)]
            lm = rng.uniform(0, 3, (m, dims[s] + 1)).astype(np.float32).astype(np.float64)
            lm[:, -1] = rng.integers(0, n_prbs + 1, m) / n_prbs
            lms.append(lm)
            cos.append(rng.normal(size=m))
        k += 1
        agents.append(dict(landmarks=lms, coeff=cos, action=rng.integers(0, n_prbs + 1, S), security_factors=rng.integers(0, 9, S),
                           margins=rng.integers(0, 5, S), adjusted=int(j & 1), accuracies=rng.uniform(0.9, 1.0, (S, n_prbs)),
                           seed=int(rng.integers(0, 2 ** 63)), tie_ctr=rng.integers(0, 100, S), prev_state=rng.uniform(0, 1, sum(dims)),
                           flags=8 * (j & 1)))
    cfg = dict(n_prbs=n_prbs, capacity=640, dims=dims, alfa=0.05, accuracy_range=(0.99, 0.999), gamma=1.0, eta=0.1)
    return cfg, agents


def all_sizes_agents():
    """seven agents: every size of SIZES in a dims-10 and in a dims-3 dictionary"""
    return make_agents(len(SIZES))


@pytest.mark.parametrize('n_agents', [1, 3, len(SIZES)])
def test_format_round_trip(n_agents):
    cfg, agents = make_agents(n_agents, seed=n_agents)
    blob = af.pack(cfg, agents)
    u = af.unpack(blob)
    assert af.pack(u) == blob and af.pack(u['config'], u['agents']) == blob
    assert u['config']['dims'] == DIMS and u['config']['n_prbs'] == N_PRBS and u['config']['capacity'] == 640
    assert len(u['agents']) == n_agents
    for a, b in zip(agents, u['agents']):
        for s in range(2):
            assert a['landmarks'][s].tobytes() == b['landmarks'][s].tobytes() and b['landmarks'][s].shape == a['landmarks'][s].shape
            assert a['coeff'][s].tobytes() == b['coeff'][s].tobytes()
        for key in ('action', 'security_factors', 'margins', 'tie_ctr'):
            assert (np.asarray(a[key]) == b[key]).all(), key
        assert a['accuracies'].tobytes() == b['accuracies'].tobytes()
        assert a['seed'] == b['seed'] and a['adjusted'] == b['adjusted'] and a['flags'] == b['flags']
        assert (a['prev_state'].astype(np.float32) == b['prev_state']).all()
        assert not b['f32bad'].any()
    if n_agents == len(SIZES):
        assert sorted(u['m'][:, 0].tolist()) == SIZES and sorted(u['m'][:, 1].tolist()) == SIZES
    # every array of the file is 8-byte aligned, the dictionaries 16
    off = af.layout(n_agents, 2, N_PRBS, 13, int((u['m'] * np.array([12, 5])).sum()))
    assert all(v % 8 == 0 for v in off.values()) and off['dict'] % 16 == 0 and off['bytes'] == len(blob)


def test_f32bad_is_found_from_the_values_and_ored_with_the_given_flag():
    cfg, agents = make_agents(len(SIZES), seed=5)    # (agent 6: 513 and 2 landmarks)
    agents[6]['landmarks'][0][3, 4] = 0.1            # not a float32 value, a state coordinate of a dims-10 dictionary
    agents[6]['landmarks'][1][0, 1] = 0.1            # dims 3: no float32 rows there
    agents[1]['f32bad'] = [0, 1]                     # a source's sticky mark travels
    u = af.unpack(af.pack(cfg, agents))
    assert u['agents'][6]['f32bad'].tolist() == [1, 0] and u['agents'][1]['f32bad'].tolist() == [0, 1]
    assert sum(int(a['f32bad'].sum()) for a in u['agents']) == 2


# ------------------------------------------------------------------ kb_agents_info (the product library, no device)
def info_code(blob):
    try:
        af.info(blob)
    except _lib.RanSliceError as e:
        return e.code, str(e)
    return 0, ''


def rehash(blob, **fields):
    """the blob with header fields replaced (by their position in the header) and the hash made right again"""
    names = ['magic', 'bytes', 'hash', 'n_agents', 'n_slices', 'n_prbs', 'capacity'] + ['dims%d' % i for i in range(8)] + \
            ['alfa', 'acc_lo', 'acc_hi', 'gamma', 'eta', 'dict_doubles']
    f = list(struct.unpack(af._HEADER, blob[:af.HEADER_BYTES]))
    for key, v in fields.items():
        f[names.index(key)] = v
    body = bytearray(blob)
    f[2] = 0
    body[:af.HEADER_BYTES] = struct.pack(af._HEADER, *f)
    f[2] = af.fnv1a(memoryview(body)[af.HASH_FROM:])
    body[:af.HEADER_BYTES] = struct.pack(af._HEADER, *f)
    return bytes(body)


@pytest.fixture(scope='module')
def good():
    cfg, agents = all_sizes_agents()
    blob = af.pack(cfg, agents)
    return cfg, agents, blob, af.unpack(blob)


def test_info_answers_a_good_blob(good):
    from ranslice.kbrl_dev import deploy_pool_bytes
    cfg, agents, blob, u = good
    i = af.info(blob)
    c = i['config']
    assert (c.n_envs, c.n_slices, c.n_prbs, c.capacity) == (len(agents), 2, N_PRBS, 640)
    assert list(c.dims) == DIMS + [0] * 6 and (c.alfa, c.acc_lo, c.acc_hi, c.gamma, c.eta) == (0.05, 0.99, 0.999, 1.0, 0.1)
    assert c.shared_dictionary == 0 and c.first_env == 0
    assert (i['m'] == u['m']).all() and i['n_agents'] == len(agents)
    assert i['pool_bytes'] == c.pool_bytes == deploy_pool_bytes(u['m']) == 512 + 15360 * int(((u['m'] + 63) // 64).sum())
    assert rehash(blob) == blob, 'the helper below restates the hash'


def boundaries(u, n_agents):
    """every byte offset at which an array of the file begins or ends"""
    m = u['m']
    off = af.layout(n_agents, 2, N_PRBS, 13, int((m * np.array([12, 5])).sum()))
    cuts = {0, af.HASH_FROM, af.HEADER_BYTES} | {v for k, v in off.items() if k != 'bytes'}
    at = off['dict']
    for j in range(n_agents):
        for s, d in enumerate((11, 4)):
            at += 8 * int(m[j, s]) * d
            cuts.add(at)
            at += 8 * int(m[j, s])
            cuts.add(at)
    assert at == off['bytes']
    cuts.discard(off['bytes'])
    return sorted(cuts), off


def test_info_refuses_truncated_blobs(good):
    cfg, agents, blob, u = good
    cuts, off = boundaries(u, len(agents))
    assert len(cuts) > 30
    for cut in cuts + [off['accuracies'] + 1001, off['dict'] + 12345]:
        code, why = info_code(blob[:cut])
        assert code == _lib.RS_EINVAL, cut
        if cut >= af.HEADER_BYTES:     # and with the header's size field made to agree, the size its other fields imply does not
            short = bytearray(blob[:cut])
            short[8:16] = struct.pack('<Q', cut)
            code, why = info_code(bytes(short))
            assert code == _lib.RS_EINVAL and 'imply' in why, (cut, why)
    assert info_code(b'')[0] == _lib.RS_EINVAL


def test_info_refuses_damaged_blobs(good):
    cfg, agents, blob, u = good
    cuts, off = boundaries(u, len(agents))
    bad = bytearray(blob)
    bad[3] ^= 0x20
    code, why = info_code(bytes(bad))
    assert code == _lib.RS_EINVAL and 'magic' in why
    # one flipped byte in each section behind the hash field: the rest of the header (a field no limit catches: eta), every
    # table, a landmark, a coefficient
    sections = [af.HEADER_BYTES - 10] + [off[k] + 2 for k in off if k not in ('bytes', 'dict')] + [off['dict'] + 8 * 12 * 1 + 3, len(blob) - 2]
    for at in sections:
        bad = bytearray(blob)
        bad[at] ^= 1
        code, why = info_code(bytes(bad))
        assert code == _lib.RS_EINVAL and 'hash' in why, (at, why)
    # fields that are consistent with the hash and wrong in themselves
    cases = dict(
        larger=(rehash(blob, n_prbs=N_PRBS + 1), 'imply'), more_agents=(rehash(blob, n_agents=len(agents) + 1), 'imply'),
        more_doubles=(rehash(blob, dict_doubles=u['m'].size * 10 ** 6), 'imply'),
        n_prbs_256=(rehash(blob, n_prbs=256), 'n_prbs <= 255'), nine_slices=(rehash(blob, n_slices=9), '<= 8 learners'),
        capacity_1=(rehash(blob, capacity=1), 'capacity'), dims_16=(rehash(blob, dims0=16), 'dimension'),
        gamma_nan=(rehash(blob, gamma=float('nan')), 'finite'), acc_inf=(rehash(blob, acc_hi=float('inf')), 'finite'),
        no_agents=(rehash(blob, n_agents=0), 'agents'))
    k = int(np.argmax(u['m'][:, 0] == 513))
    for name, m_bad in (('m_beyond_capacity', 641), ('m_negative', -1)):
        b = bytearray(blob)
        b[off['m'] + 8 * k:off['m'] + 8 * k + 4] = struct.pack('<i', m_bad)
        cases[name] = (rehash(bytes(b)), 'capacity')
    b = bytearray(blob)
    b[off['m'] + 8 * k:off['m'] + 8 * k + 4] = struct.pack('<i', 512)     # within the limits, but the sizes no longer add up
    cases['m_other'] = (rehash(bytes(b)), 'add up')
    b = bytearray(blob)
    b[off['action']:off['action'] + 4] = struct.pack('<i', N_PRBS + 1)
    cases['action'] = (rehash(bytes(b)), 'action')
    for name, (b, word) in cases.items():
        code, why = info_code(b)
        assert code == _lib.RS_EINVAL and word in why, (name, why)
    assert info_code(blob) == (0, ''), 'and the good blob is still good'


# ------------------------------------------------------------------ the reference's own agents
@pytest.fixture(scope='module', params=ar.FIXTURES)
def fixture(request, golden_dir):
    return ar.Fixture(golden_dir, request.param)


def test_restatement_gives_what_the_reference_recorded(fixture):
    """select_action restated in float64 on the FINAL dictionaries and final_state gives the recorded last action, margins and
    adjusted flag; no scanned candidate's |f| lies within 100 tolerances of zero (measured: the smallest ratio over the four
    fixtures is 2.7e3, g10_kbrl_s2)"""
    fx = fixture
    r = ar.select_action(fx, fx.final_state)
    print('%s: smallest |f| / tol over the scanned candidates %.4g' % (fx.name, r['ratio'].min()))
    assert (r['action'] == fx.action).all() and r['adjusted'] == fx.adjusted and (r['margins'] == fx.margins).all()
    assert r['ratio'].min() >= 100.0
    for s in range(fx.S):
        lm = fx.landmarks[s]
        st = lm[:, :-1]
        assert (st.astype(np.float32).astype(np.float64) == st).all(), 'every state coordinate of a landmark is a float32 value'
        a = np.rint(lm[:, -1] * fx.n_prbs)
        assert ((a >= 0) & (a <= fx.n_prbs) & (a / fx.n_prbs == lm[:, -1])).all(), 'every landmark is on the candidate grid'


def as_reference_agent(fx):
    """an object shaped like the reference's KBRL_Control around the fixture's arrays"""
    learners, at = [], 0
    for s in range(fx.S):
        sv = types.SimpleNamespace(landmarks=fx.landmarks[s], coeff=fx.coeff[s], counter=fx.landmarks[s].shape[0])
        alg = types.SimpleNamespace(sv=sv, eta=ar.ETA, kernel=types.SimpleNamespace(sv=sv, gamma=ar.GAMMA))
        learners.append(types.SimpleNamespace(algorithm=alg, indexes=np.arange(at, at + fx.dims[s])))
        at += fx.dims[s]
    return types.SimpleNamespace(learners=learners, n_prbs=fx.n_prbs, alfa=ar.ALFA, accuracy_range=list(fx.a_range),
                                 adjusted=fx.adjusted, action=fx.action.astype(np.int16), margins=fx.margins.astype(np.int16),
                                 security_factors=fx.security.astype(np.int16), accuracies=fx.acc)


def test_from_reference_packs_a_duck_typed_agent(fixture):
    fx = fixture
    blob = af.from_reference(as_reference_agent(fx))
    assert blob == af.pack(fx.config(), [fx.agent()])
    i = af.info(blob)
    assert i['m'].tolist() == [[lm.shape[0] for lm in fx.landmarks]] and i['config'].n_prbs == fx.n_prbs
    two = af.unpack(af.from_reference([as_reference_agent(fx)] * 2, seeds=[7, 9]))
    assert [a['seed'] for a in two['agents']] == [7, 9]
    # a single landmark is a 1-D array in the reference, a dictionary before its first insert has none
    ag = as_reference_agent(fx)
    ag.learners[0].algorithm.sv = types.SimpleNamespace(landmarks=fx.landmarks[0][0], coeff=np.array([1.0], dtype=np.float32), counter=1)
    ag.learners[1].algorithm.sv = types.SimpleNamespace(counter=0)
    u = af.unpack(af.from_reference(ag))
    assert u['m'][0, :2].tolist() == [1, 0] and u['agents'][0]['landmarks'][0].shape == (1, fx.dims[0] + 1)
