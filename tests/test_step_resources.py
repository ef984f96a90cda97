"""The step kernel's register budget as the last build reports it (csrc/build/resources.log and the device listing
csrc/build/rs_api.s, read through tools/check_resources.py and tools/spill_sites.py): the production instance keeps its
allocation -- 96 VGPRs, 5 waves per SIMD, LDS for five blocks per CU, no more scratch than before the launch constants left the
spilled SGPRs -- spills fewer SGPRs than the 137 it did then, no more than the ceiling check_resources.py holds it to, and
reloads none of them inside the fast reception round loop or the PF leader-run loop; the spill columns are there for every
instance of the template."""
import contextlib
import importlib.util
import io
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_SGPR_SPILL = 137   # <16, false, false, true> before this budget was kept (profiles/step_sgpr_ab.txt)
PLAIN_SCRATCH, BLOCK_SCRATCH = 112, 160   # B per lane, the same two instances then


@pytest.fixture(scope='module')
def cr():
    spec = importlib.util.spec_from_file_location('check_resources', os.path.join(ROOT, 'tools', 'check_resources.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert os.path.exists(m.LOG), 'no %s: build first (__graft_entry__.build)' % m.LOG
    return m


def test_production_instance_keeps_its_allocation(cr):
    inst = cr.step_instances(cr.parse())
    plain, block = inst['ILi16ELb0ELb0ELb1E'], inst['ILi16ELb0ELb1ELb1E']
    assert plain['VGPRs'] == 96 and plain['Occupancy'] == 5
    assert plain['LDS Size'] <= 32768 and block['LDS Size'] <= 32768
    assert plain['ScratchSize'] <= PLAIN_SCRATCH
    assert block['ScratchSize'] <= BLOCK_SCRATCH and block['Occupancy'] == 5
    assert plain['SGPRs Spill'] < PARENT_SGPR_SPILL
    assert plain['SGPRs Spill'] <= cr.SGPR_SPILL_CEILING < PARENT_SGPR_SPILL


def test_spill_columns_for_every_step_instance(cr):
    inst = cr.step_instances(cr.parse())
    # 8, 16 and 32 lanes; tracing, BLOCK and plain; both values of FDIV wherever rs_api.hip launches both
    want = {'ILi%dELb%dELb%dELb%dE' % (g, t, b, f) for g in (8, 16, 32) for t, b in ((1, 1), (0, 1)) for f in (0, 1)}
    want |= {'ILi%dELb0ELb0ELb%dE' % (g, f) for g in (8, 16) for f in (0, 1)}
    assert want <= set(inst), sorted(want - set(inst))
    for targs, r in inst.items():
        for col in ('VGPRs', 'ScratchSize', 'Occupancy', 'SGPRs Spill', 'VGPRs Spill', 'LDS Size'):
            assert col in r, (targs, col)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        problems = cr.check()
    assert problems == []
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith('embb_step_kernelIL') and 'VGPRs ' in ln]
    assert len(lines) == len(inst)
    for ln in lines:
        assert 'SGPRs spilled' in ln and 'VGPRs spilled' in ln and 'None' not in ln, ln


def test_hottest_loops_hold_no_spill_reload(cr):
    """the fast reception round loop and the PF leader-run loop of the production instance, found in the build's own listing by
    what they hold; a signature that matches nothing, or a loop of another size, fails as a reload does"""
    assert os.path.exists(cr.LISTING), 'no %s: build first (__graft_entry__.build)' % cr.LISTING
    assert os.path.getmtime(cr.LISTING) >= os.path.getmtime(cr.LOG) - 600, 'the listing is older than the library it should describe'
    spec = importlib.util.spec_from_file_location('spill_sites', os.path.join(ROOT, 'tools', 'spill_sites.py'))
    ss = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ss)
    assert ss.check_step_loops(cr.LISTING, cr.PLAIN) == []
    res = ss.analyse(cr.LISTING, cr.PLAIN)
    for label, sig in ss.STEP_LOOPS.items():
        span = ss.innermost_loop_with(res, sig.split(','))
        lo, hi = ss.STEP_LOOP_SIZE[label]
        assert span is not None and lo <= span[1] - span[0] + 1 <= hi, label
        assert ss.reloads_in(res, span) == [], label
