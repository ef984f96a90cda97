"""Agent files ("KBAGENT1") on the host: the bytes kb_export_agents writes and kb_import_agents reads (include/ranslice.h,
csrc/kb_agents.hip), from and to plain numpy arrays.  numpy only: no device, no torch; info() alone calls the
library (kb_agents_info, which makes no device call).

    unpack(blob)            -> dict(config=..., agents=[...], m=[n, S])
    pack(config, agents)    -> bytes, the device's bytes exactly, hash included; pack(unpack(blob)) == blob
    info(blob)              -> the configuration and pool kb_import_agents would create, validated by the library
    from_reference(agent)   -> bytes, from anything shaped like the reference's kbrl_control.KBRL_Control
    with_capacity(blob, c)  -> bytes, the same agents under another capacity (room to grow for imported learners)

config: dict(n_prbs, capacity, dims [S], alfa, accuracy_range (lo, hi), gamma, eta).
An agent: dict(landmarks = S arrays [m, dims[s] + 1], coeff = S arrays [m], action, security_factors, margins [S], adjusted,
accuracies [S, n_prbs], seed, tie_ctr [S], prev_state [sum(dims)], flags, f32bad [S]); the last five are optional (zeros;
f32bad is found from the values and ORed with what is given, as the device does when it builds the pages).

The hash is FNV-1a over every byte behind the hash field, in a Python loop here: fine for agents of a few thousand landmarks
(about a second per 5 MB); fleets are exported on the device (VecKBRL.export_agents)."""
import ctypes as C
import struct

import numpy as np

MAGIC = b'KBAGENT1'
HEADER_BYTES = 120
HASH_FROM = 24
MAX_SLICES = 8
_HEADER = '<8sQQ4i8i5dQ'   # magic, bytes, hash, n_agents, n_slices, n_prbs, capacity, dims[8], alfa, acc_lo, acc_hi, gamma, eta, doubles
assert struct.calcsize(_HEADER) == HEADER_BYTES

_FNV_BASIS, _FNV_PRIME, _M64 = 1469598103934665603, 1099511628211, (1 << 64) - 1


def fnv1a(data, h=_FNV_BASIS):
    """FNV-1a, 64 bit (csrc/rs_host.h: fnv1a)"""
    for b in bytes(data):
        h = ((h ^ b) * _FNV_PRIME) & _M64
    return h


# the tables, in file order: (name, dtype, shape per agent as a function of (S, n_prbs, nv))
_TABLES = (('m', '<i4', lambda S, P, nv: (S,)), ('f32bad', '<i4', lambda S, P, nv: (S,)),
           ('action', '<i4', lambda S, P, nv: (S,)), ('security_factors', '<i4', lambda S, P, nv: (S,)),
           ('margins', '<i4', lambda S, P, nv: (S,)), ('adjusted', '<i4', lambda S, P, nv: ()),
           ('accuracies', '<f8', lambda S, P, nv: (S, P)), ('seed', '<u8', lambda S, P, nv: ()),
           ('tie_ctr', '<u4', lambda S, P, nv: (S,)), ('prev_state', '<f4', lambda S, P, nv: (nv,)),
           ('flags', '<i4', lambda S, P, nv: ()))


def layout(n, S, n_prbs, nv, dict_doubles):
    """byte offsets of the tables and of the dictionaries, and the file's size: every table 8-byte aligned, the dictionaries
    16-byte aligned (csrc/kb_agents.hip: kb_agents_layout_of)"""
    at, off = HEADER_BYTES, {}
    for key, dt, shape in _TABLES:
        off[key] = at
        at = (at + n * int(np.prod(shape(S, n_prbs, nv), dtype=np.int64)) * np.dtype(dt).itemsize + 7) & ~7
    at = (at + 15) & ~15
    off['dict'] = at
    off['bytes'] = at + 8 * dict_doubles
    return off


def _config(cfg):
    dims = [int(d) for d in cfg['dims']]
    lo, hi = cfg['accuracy_range']
    return dict(n_prbs=int(cfg['n_prbs']), capacity=int(cfg['capacity']), dims=dims, alfa=float(cfg['alfa']),
                accuracy_range=(float(lo), float(hi)), gamma=float(cfg['gamma']), eta=float(cfg['eta']))


def pack(config, agents=None):
    """-> the file as bytes.  pack(config, agents), or pack(u) with u = unpack(blob)"""
    if agents is None:
        config, agents = config['config'], config['agents']
    cfg = _config(config)
    dims, P = cfg['dims'], cfg['n_prbs']
    S, nv, n = len(dims), sum(dims), len(agents)
    if not (0 < S <= MAX_SLICES) or n <= 0:
        raise ValueError('agent_file.pack: between 1 and %d learners per agent and at least one agent' % MAX_SLICES)
    cols = {key: np.zeros((n,) + shape(S, P, nv), dtype=dt) for key, dt, shape in _TABLES}
    parts = []
    for j, ag in enumerate(agents):
        for s in range(S):
            d = dims[s] + 1
            lm = np.ascontiguousarray(ag['landmarks'][s], dtype='<f8').reshape(-1, d)
            co = np.ascontiguousarray(ag['coeff'][s], dtype='<f8').reshape(-1)
            if lm.shape[0] != co.shape[0]:
                raise ValueError('agent_file.pack: agent %d, learner %d: %d landmarks, %d coefficients' % (j, s, lm.shape[0], co.shape[0]))
            cols['m'][j, s] = lm.shape[0]
            if dims[s] == 10 and lm.size:   # a state coordinate that is no float32 value (csrc/kb_kbrl.hip: KB_ROW_F32)
                with np.errstate(invalid='ignore', over='ignore'):
                    cols['f32bad'][j, s] = int((lm[:, :10].astype(np.float32).astype(np.float64) != lm[:, :10]).any())
            parts += [lm.tobytes(), co.tobytes()]
        if ag.get('f32bad') is not None:
            cols['f32bad'][j] |= (np.asarray(ag['f32bad']).reshape(S) != 0).astype(np.int32)
        for key in ('action', 'security_factors', 'margins', 'adjusted', 'accuracies'):
            cols[key][j] = np.asarray(ag[key]).reshape(cols[key][j].shape)
        for key in ('seed', 'tie_ctr', 'prev_state', 'flags'):
            if ag.get(key) is not None:
                cols[key][j] = np.asarray(ag[key]).reshape(cols[key][j].shape)
    doubles = int((cols['m'].astype(np.int64) * (np.asarray(dims, dtype=np.int64) + 2)[None, :]).sum())
    off = layout(n, S, P, nv, doubles)
    out = bytearray(off['bytes'])
    for key, _, _ in _TABLES:
        raw = cols[key].tobytes()
        out[off[key]:off[key] + len(raw)] = raw
    out[off['dict']:] = b''.join(parts)
    assert len(out) == off['bytes']

    def header(h):
        return struct.pack(_HEADER, MAGIC, off['bytes'], h, n, S, P, cfg['capacity'], *(dims + [0] * (MAX_SLICES - S)), cfg['alfa'],
                           cfg['accuracy_range'][0], cfg['accuracy_range'][1], cfg['gamma'], cfg['eta'], doubles)
    out[:HEADER_BYTES] = header(0)
    out[:HEADER_BYTES] = header(fnv1a(memoryview(out)[HASH_FROM:]))
    return bytes(out)


def read_header(blob):
    """the header's fields as a dict (no validation beyond its length: info() validates)"""
    f = struct.unpack(_HEADER, bytes(blob[:HEADER_BYTES]))
    S = f[4]
    return dict(magic=f[0], bytes=f[1], hash=f[2], n_agents=f[3], n_slices=S, n_prbs=f[5], capacity=f[6], dims=list(f[7:15]),
                alfa=f[15], accuracy_range=(f[16], f[17]), gamma=f[18], eta=f[19], dict_doubles=f[20])


def with_capacity(blob, capacity):
    """-> the same file with the header's capacity replaced (and the hash with it): the limit per dictionary of the handle an
    import creates.  VecKBRL.load_agents(blob, learning=True, capacity=...) uses it to give imported learners room to grow."""
    blob = bytes(blob)
    f = list(struct.unpack(_HEADER, blob[:HEADER_BYTES]))
    if f[0] != MAGIC:
        raise ValueError('agent_file.with_capacity: not an agent file')
    if int(capacity) == f[6]:
        return blob
    f[6] = int(capacity)
    f[2] = 0
    out = bytearray(blob)
    out[:HEADER_BYTES] = struct.pack(_HEADER, *f)
    f[2] = fnv1a(memoryview(out)[HASH_FROM:])
    out[:HEADER_BYTES] = struct.pack(_HEADER, *f)
    return bytes(out)


def unpack(blob, check=True):
    """-> dict(config, agents, m).  check: the magic, the size and the hash (ValueError); the library's kb_agents_info is the
    validator of untrusted bytes (info())"""
    blob = bytes(blob)
    if len(blob) < HEADER_BYTES:
        raise ValueError('agent_file.unpack: shorter than the header')
    h = read_header(blob)
    S, P, n = h['n_slices'], h['n_prbs'], h['n_agents']
    if h['magic'] != MAGIC or not (0 < S <= MAX_SLICES) or n <= 0 or P <= 0:
        raise ValueError('agent_file.unpack: not an agent file')
    dims = h['dims'][:S]
    nv = sum(dims)
    off = layout(n, S, P, nv, h['dict_doubles'])
    if check and (off['bytes'] != len(blob) or h['bytes'] != len(blob)):
        raise ValueError('agent_file.unpack: the header implies %d bytes, the blob has %d' % (off['bytes'], len(blob)))
    if check and fnv1a(memoryview(blob)[HASH_FROM:]) != h['hash']:
        raise ValueError('agent_file.unpack: the hash does not match the contents')
    cols = {}
    for key, dt, shape in _TABLES:
        shp = (n,) + shape(S, P, nv)
        cols[key] = np.frombuffer(blob, dtype=dt, count=int(np.prod(shp, dtype=np.int64)), offset=off[key]).reshape(shp).copy()
    agents, at = [], off['dict']
    for j in range(n):
        lms, cos = [], []
        for s in range(S):
            m, d = int(cols['m'][j, s]), dims[s] + 1
            if m < 0 or at + 8 * m * (d + 1) > len(blob):
                raise ValueError('agent_file.unpack: a dictionary runs past the end of the blob')
            lms.append(np.frombuffer(blob, dtype='<f8', count=m * d, offset=at).reshape(m, d).copy())
            cos.append(np.frombuffer(blob, dtype='<f8', count=m, offset=at + 8 * m * d).copy())
            at += 8 * m * (d + 1)
        ag = dict(landmarks=lms, coeff=cos, adjusted=int(cols['adjusted'][j]), seed=int(cols['seed'][j]), flags=int(cols['flags'][j]))
        for key in ('f32bad', 'action', 'security_factors', 'margins', 'accuracies', 'tie_ctr', 'prev_state'):
            ag[key] = cols[key][j]
        agents.append(ag)
    cfg = dict(n_prbs=P, capacity=h['capacity'], dims=dims, alfa=h['alfa'], accuracy_range=h['accuracy_range'], gamma=h['gamma'],
               eta=h['eta'])
    return dict(config=cfg, agents=agents, m=cols['m'])


def info(blob, lib=None):
    """validate a blob with the library (kb_agents_info: host only, no device call) -> dict(config = the KbConfig
    kb_import_agents would create, n_agents, pool_bytes, m [n, S]); raises ranslice._lib.RanSliceError(RS_EINVAL, reason)"""
    from . import _lib
    from .config import KbConfig
    L = lib if lib is not None else _lib.load()
    raw = np.frombuffer(bytes(blob), dtype=np.uint8)
    cfg = KbConfig()
    ptr = raw.ctypes.data_as(C.c_void_p) if raw.size else None
    rc = L.kb_agents_info(ptr, raw.size, C.byref(cfg), None)
    if rc != 0:
        raise _lib.RanSliceError(rc, L.kb_last_error(None).decode())
    m = np.zeros((cfg.n_envs, cfg.n_slices), dtype=np.int32)
    rc = L.kb_agents_info(ptr, raw.size, C.byref(cfg), m.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise _lib.RanSliceError(rc, L.kb_last_error(None).decode())
    return dict(config=cfg, n_agents=int(cfg.n_envs), pool_bytes=int(cfg.pool_bytes), m=m)


def from_reference(agent, seeds=None, capacity=None):
    """-> the file of one agent, or of a list of agents, shaped like the reference's KBRL_Control: .learners[i].algorithm.sv
    (.landmarks, .coeff), .algorithm.eta, .algorithm.kernel.gamma, .learners[i].indexes, .security_factors, .margins, .action,
    .adjusted, .accuracies, .accuracy_range, .alfa, .n_prbs.  Nothing of the reference is imported.  seeds: the tie-break
    streams' seeds (default 0, 1, ...: the reference draws its ties from numpy's global generator, which no file can carry).
    capacity: the deployed handle's limit (default: the largest dictionary, at least 64, rounded up to 64 landmarks)."""
    agents = list(agent) if isinstance(agent, (list, tuple)) else [agent]
    first = agents[0]
    S = len(first.learners)
    dims, at = [], 0
    for h in first.learners:
        idx = [int(i) for i in np.asarray(h.indexes).reshape(-1)]
        if idx != list(range(at, at + len(idx))):
            raise ValueError('agent_file.from_reference: the learners must read consecutive runs of the state, in order')
        dims.append(len(idx))
        at += len(idx)
    algs = [h.algorithm for a in agents for h in a.learners]
    gammas, etas = {float(g.kernel.gamma) for g in algs}, {float(g.eta) for g in algs}
    if len(gammas) != 1 or len(etas) != 1:
        raise ValueError('agent_file.from_reference: one gamma and one eta for all learners')
    out, largest = [], 0
    for k, a in enumerate(agents):
        if len(a.learners) != S or int(a.n_prbs) != int(first.n_prbs):
            raise ValueError('agent_file.from_reference: agents of one file share their configuration')
        lms, cos = [], []
        for s, h in enumerate(a.learners):
            sv, d = h.algorithm.sv, dims[s] + 1
            if getattr(sv, 'counter', 0) == 0 or not hasattr(sv, 'landmarks'):   # (SVvariable before its first insert)
                lm, co = np.zeros((0, d)), np.zeros(0)
            else:
                lm = np.asarray(sv.landmarks, dtype=np.float64).reshape(-1, d)   # (one landmark is a 1-D array there)
                co = np.asarray(sv.coeff, dtype=np.float64).reshape(-1)
            lms.append(lm)
            cos.append(co)
            largest = max(largest, lm.shape[0])
        out.append(dict(landmarks=lms, coeff=cos, action=np.asarray(a.action), security_factors=np.asarray(a.security_factors),
                        margins=np.asarray(a.margins), adjusted=int(a.adjusted), accuracies=np.asarray(a.accuracies, dtype=np.float64),
                        seed=int(seeds[k]) if seeds is not None else k))
    if capacity is None:
        capacity = max(64, (largest + 63) // 64 * 64)
    cfg = dict(n_prbs=int(first.n_prbs), capacity=int(capacity), dims=dims, alfa=float(first.alfa),
               accuracy_range=(float(first.accuracy_range[0]), float(first.accuracy_range[1])), gamma=gammas.pop(), eta=etas.pop())
    return pack(cfg, out)
