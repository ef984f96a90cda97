"""The C-ABI library loads and exports every symbol include/ranslice.h declares (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b((?:rs|kb)_[a-z_0-9]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    from ranslice import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libranslice.so not built (python __graft_entry__.py build)')
    lib = C.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(_lib.EXPORTS) == set(names)


def test_config_struct_matches_header():
    """field order of the ctypes mirrors == the C structs (guards against silent ABI drift)"""
    from ranslice.config import RsConfig, KbConfig, RsAllocRec
    text = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()

    def fields(struct):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        out = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            decl = re.sub(r'^(int32_t|int64_t|double|float|uint64_t)\s+', '', decl)
            for name in decl.split(','):
                out.append(re.sub(r'\[.*\]', '', name).strip())
        return out
    assert fields('rs_config') == [f[0] for f in RsConfig._fields_]
    assert fields('kb_config') == [f[0] for f in KbConfig._fields_]
    assert fields('rs_alloc_rec') == [f[0] for f in RsAllocRec._fields_]
    assert C.sizeof(RsAllocRec) == 48


def test_product_has_no_oracle_dependency():
    """nothing under network-slicing_amd/ may import or link the oracle"""
    pkg = os.path.join(ROOT, 'network-slicing_amd')
    for dp, dn, fn in os.walk(pkg):
        if 'build' in dp:
            continue
        for f in fn:
            if f.endswith(('.py', '.hip', '.h')):
                src = open(os.path.join(dp, f)).read()
                assert 'pyoracle' not in src and 'rs_oracle' not in src and 'kb_oracle' not in src, f


def test_production_instances_keep_their_register_budget():
    """the two 16-lane production instances of the step kernel must stay at 5 waves per SIMD and below 240 B of
    spills per lane (tools/check_resources.py reads the remarks of the last build)"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log = os.path.join(root, 'network-slicing_amd', 'csrc', 'build', 'resources.log')
    if not os.path.exists(log):
        import pytest
        pytest.skip('no build log (library built without the Makefile)')
    spec = importlib.util.spec_from_file_location('check_resources', os.path.join(root, 'tools', 'check_resources.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.check(log) == []


def test_production_library_reads_no_developer_knob():
    """the sweep switches, the guard bands and the fault injector of the shared step live in the test build only
    (csrc/rs_api.hip: dev_env, -DRS_DEV): none of their names is even a string of libranslice.so, all of them are in
    libranslice_dev.so; the variables the product does read are documented ones"""
    from ranslice import _lib
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.DEV_LIB_PATH)):
        pytest.skip('libraries not built')
    prod = open(_lib.LIB_PATH, 'rb').read()
    dev = open(_lib.DEV_LIB_PATH, 'rb').read()
    knobs = [b'KBRL_INJECT_FAIL_ROUND', b'KBRL_ROUNDS', b'KBRL_STREAM_GRID', b'KBRL_HEAVY_M', b'KBRL_SERIAL_APPLY', b'RANSLICE_SNAKE', b'RANSLICE_KEY_W',
             b'RANSLICE_PAIR', b'RANSLICE_ORDER', b'RANSLICE_GUARD', b'RANSLICE_EXACT_DIV', b'RANSLICE_HINT']
    for k in knobs:   # (as a whole NUL-terminated string: the argument of a getenv)
        assert k + b'\0' not in prod, k
        assert k + b'\0' in dev, k
    # the primitive probe (csrc/rs_probe.hip) is test tooling too: neither the entry point nor its kernels are in the product
    # and so are the accessors of the agent's scoring chain (csrc/kb_probe.hip)
    for k in (b'rs_dev_probe', b'probe_kernel', b'kb_dev_get_scores', b'kb_dev_get_rows', b'kb_dev_get_update_rows',
              b'kb_dev_get_shared_scores', b'kb_dev_get_shared_apply', b'kb_dev_get_prune_grid'):
        assert k not in prod, k
        assert k in dev, k
    assert not [n for n in _lib.EXPORTS if '_dev_' in n]
    for k in (b'RANSLICE_RCCL_LIB', b'KBRL_COLLECTIVE_TIMEOUT_S'):
        assert k in prod, k
    src = ''.join(open(os.path.join(ROOT, 'network-slicing_amd', 'csrc', f)).read() for f in ('rs_api.hip', 'kb_api.hip'))
    assert sorted(set(re.findall(r'[^_]getenv\("([A-Z_0-9]+)"\)', src))) == ['KBRL_COLLECTIVE_TIMEOUT_S', 'RANSLICE_RCCL_LIB',
                                                                             'ROCP_TOOL_LIBRARIES']
