"""While a handle's lanes are open its lanes' streams are not joined: an entry point that touched the handle's buffers or
its main stream then would race with them.  So every extern "C" function of csrc/*.hip that takes an rs_handle* must name the
close helper (lanes_close), or one of the two lane-aware helpers (lanes_actions, lanes_step), in its body.  A new entry
point that forgets to join fails here.  No GPU."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'network-slicing_amd', 'csrc')

HELPERS = ('lanes_close', 'lanes_actions', 'lanes_step')
# pure getters of host fields that no launch writes
EXEMPT = ('rs_last_error', 'rs_n_vars', 'rs_n_slices')


def _strip_comments(text):
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    return re.sub(r'//[^\n]*', ' ', text)


def _body(text, open_brace):
    depth = 0
    for i in range(open_brace, len(text)):
        if text[i] == '{':
            depth += 1
        elif text[i] == '}':
            depth -= 1
            if depth == 0:
                return text[open_brace:i + 1]
    raise AssertionError('unbalanced braces')


def _entry_points():
    """(file, name, body) of every extern "C" definition with an rs_handle* parameter"""
    found = []
    for path in sorted(glob.glob(os.path.join(CSRC, '*.hip'))):
        text = _strip_comments(open(path).read())
        for m in re.finditer(r'extern\s+"C"\s+[\w\s\*]*?\b(\w+)\s*\(([^()]*)\)\s*\{', text):
            name, params = m.group(1), m.group(2)
            if re.search(r'\brs_handle\s*\*\s*\w', params):     # (rs_create's rs_handle** out is no handle yet)
                found.append((os.path.basename(path), name, _body(text, m.end() - 1)))
    return found


def test_the_scan_finds_the_entry_points():
    names = {n for _, n, _ in _entry_points()}
    assert len(names) >= 40
    for n in ('rs_fetch', 'rs_step', 'rs_step_resident', 'rs_random_actions', 'rs_run_random', 'rs_save_state', 'rs_load_state',
              'rs_reset', 'rs_destroy', 'rs_fork', 'rs_step_device', 'rs_set_lanes', 'rs_get_lane_info', 'kb_step_resident',
              'kb_run_resident', 'kb_shared_step_resident') + EXEMPT:
        assert n in names, n
    assert 'rs_create' not in names


def test_every_entry_point_joins_the_lanes():
    missing = [(f, n) for f, n, body in _entry_points()
               if n not in EXEMPT and not any(re.search(r'\b%s\s*\(' % h, body) for h in HELPERS)]
    assert not missing, 'entry points that neither close the lanes nor step them: %s' % missing


def test_a_forgetful_entry_point_is_caught(tmp_path, monkeypatch):
    """the scan on a source that forgets: the test above would fail for it"""
    src = tmp_path / 'x.hip'
    src.write_text('extern "C" int rs_new_thing(rs_handle* h, int k) {\n    // lanes_close(h) in a comment does not count\n'
                   '    if (!h) return -1;\n    return k;\n}\n'
                   'extern "C" int rs_other(const double* p,\n                        rs_handle* env) {\n'
                   '    if (lanes_close(env) != 0) return -3;\n    return 0;\n}\n')
    monkeypatch.setattr(sys.modules[__name__], 'CSRC', str(tmp_path))
    eps = _entry_points()
    assert [n for _, n, _ in eps] == ['rs_new_thing', 'rs_other']
    assert [any(re.search(r'\b%s\s*\(' % h, b) for h in HELPERS) for _, _, b in eps] == [False, True]
