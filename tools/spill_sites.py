#!/usr/bin/env python3
"""Where a kernel reloads spilled SGPRs: the reload sites of one function of a gfx950 assembly listing, by loop depth.

The back end parks SGPRs it cannot keep in lanes of a VGPR (v_writelane_b32) and fetches them back with v_readlane_b32; each
reload is a VALU issue slot, and the parking VGPRs are lost to the allocation.  resources.log counts the spilled SGPRs but not
where they come back; this reads the listing:

    make -C network-slicing_amd/csrc asm          # build/rs_api.s, compiled as the product is
    python tools/spill_sites.py network-slicing_amd/csrc/build/rs_api.s embb_step_kernelILi16ELb0ELb0ELb1E --step-loops [--sites]

Spill VGPRs are the destinations of v_writelane_b32 (the step kernel's source has no write-lane of its own); a reload is a
v_readlane_b32 from one of them.  Loops are the spans between a label and a later branch back to it.  The product's listing has
no line tables (-gline-tables-only changes the step kernel's allocation: scratch 112 -> 152 B per lane), so a loop is named by
what it holds: --loop-with takes mnemonic prefixes (`name*N`: at least N, `!name`: none) and reports the smallest loop that
fits; --step-loops are the two of the step kernel that DESIGN.md section 4 holds to no reload.  --loop-at FILE:LINE works on a
listing made with line tables (an approximation of the product's allocation).
"""
import argparse
import re
import sys


def function_lines(path, key):
    """the listing of the first function whose symbol contains `key`, and the .file table"""
    files, body, name = {}, None, None
    for line in open(path, errors='replace'):
        m = re.match(r'\s*\.file\s+(\d+)\s+(?:"[^"]*"\s+)?"([^"]*)"', line)
        if m:
            files[int(m.group(1))] = m.group(2).rsplit('/', 1)[-1]
        if body is None:
            m = re.match(r'(\S+):\s', line)
            if m and key in m.group(1) and not m.group(1).startswith('.'):
                name, body = m.group(1), []
            continue
        if re.match(r'\s*\.end_amdhsa_kernel|\s*\.size\s+' + re.escape(name), line) or line.startswith('.Lfunc_end'):
            break
        body.append(line.rstrip('\n'))
    if body is None:
        raise SystemExit('%s: no function matching %s' % (path, key))
    return name, body, files


def analyse(path, key):
    name, body, files = function_lines(path, key)
    insts = []     # (mnemonic, operands, (file, line))
    labels = {}    # label -> index of the next instruction
    loc = (None, 0)
    for line in body:
        s = line.split(';', 1)[0].strip()
        if not s:
            continue
        m = re.match(r'\.loc\s+(\d+)\s+(\d+)', s)
        if m:
            loc = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
            continue
        m = re.match(r'(\.LBB\w+):', s)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        if s.startswith('.') or s.endswith(':'):
            continue
        parts = s.split(None, 1)
        insts.append((parts[0], parts[1] if len(parts) > 1 else '', loc))
    loops = {}     # header index -> last index of a branch back to it
    for i, (mn, ops, _) in enumerate(insts):
        if mn.startswith('s_cbranch') or mn == 's_branch':
            t = labels.get(ops.strip())
            if t is not None and t <= i:
                loops[t] = max(loops.get(t, i), i)
    spans = sorted(loops.items())
    spill_regs = set()
    for mn, ops, _ in insts:
        if mn == 'v_writelane_b32':
            spill_regs.add(ops.split(',')[0].strip())
    reloads, stores = [], []
    for i, (mn, ops, lc) in enumerate(insts):
        o = [x.strip() for x in ops.split(',')]
        if mn == 'v_readlane_b32' and len(o) >= 3 and o[1] in spill_regs:
            reloads.append((i, o[1], o[2], lc))
        if mn == 'v_writelane_b32':
            stores.append((i, o[0], o[2] if len(o) > 2 else '?', lc))

    def enclosing(i):
        return [(a, b) for a, b in spans if a <= i <= b]

    return dict(name=name, insts=insts, spans=spans, spill_regs=sorted(spill_regs), reloads=reloads, stores=stores, enclosing=enclosing)


def innermost_loop_at(res, fname, line):
    best = None
    for i, (_, _, lc) in enumerate(res['insts']):
        if lc[0] == fname and lc[1] == line:
            enc = res['enclosing'](i)
            if enc:
                inner = min(enc, key=lambda ab: ab[1] - ab[0])
                if best is None or inner[1] - inner[0] < best[1] - best[0]:
                    best = inner
    return best


def innermost_loop_with(res, wants):
    """the smallest loop that holds every given mnemonic (prefix match; `name*N`: at least N of them; `!name`: none of them): how a
    loop is named without line tables"""
    need, ban = {}, []
    for w in wants:
        if w.startswith('!'):
            ban.append(w[1:])
            continue
        name, _, n = w.partition('*')
        need[name] = int(n or 1)
    best = None
    for a, b in res['spans']:
        have = dict.fromkeys(need, 0)
        ok = True
        for mn, _, _ in res['insts'][a:b + 1]:
            if any(mn.startswith(x) for x in ban):
                ok = False
                break
            for name in need:
                if mn.startswith(name):
                    have[name] += 1
        if ok and all(have[k] >= need[k] for k in need) and (best is None or b - a < best[1] - best[0]):
            best = (a, b)
    return best


# the step kernel's two hottest inner loops, by what they hold:
STEP_LOOPS = {
    # fast_team_sums' round loop: eight owners by s_ff1, float32 sigmoids, no call (team_response's round loop calls rs_exp2_ool)
    'fast reception round loop': 'v_exp_f32,s_ff1_i32_b64*8,!s_swappc',
    # the PF leader's run: min / multiply of the RB pair, the share's two fmas, no memory access of any kind
    'PF leader-run loop': 'v_fma_f64*2,v_mul_lo_u32,v_cvt_f64_i32,v_min_i32,!global_,!ds_,!v_exp_f32,!s_swappc',
}


def reloads_in(res, span):
    return [r for r in res['reloads'] if span[0] <= r[0] <= span[1]]


# plausible sizes of the two loops in instructions (318 / 56 in the parent of the no-reload rule, 310 / 68 in the build that set
# it): a signature that lands on some other loop after a scheduling change should fail loudly rather than vouch for the wrong code
STEP_LOOP_SIZE = {'fast reception round loop': (250, 400), 'PF leader-run loop': (40, 110)}


def check_step_loops(listing, kernel):
    """problems (strings) with the no-reload rule of the step kernel's two hottest loops: a loop that no longer matches its
    signature, matches at an implausible size, or holds a spill reload"""
    res = analyse(listing, kernel)
    bad = []
    for label, spec in STEP_LOOPS.items():
        span = innermost_loop_with(res, spec.split(','))
        if span is None:
            bad.append('%s: %s: no loop fits its signature (%s) -- update tools/spill_sites.py: STEP_LOOPS' % (kernel, label, spec))
            continue
        n, (lo, hi) = span[1] - span[0] + 1, STEP_LOOP_SIZE[label]
        if not lo <= n <= hi:
            bad.append('%s: %s: the signature matches a loop of %d instructions, expected %d..%d -- wrong loop?' % (kernel, label, n, lo, hi))
            continue
        rl = reloads_in(res, span)
        if rl:
            bad.append('%s: %s (%d instructions) holds %d SGPR spill reloads: %s' % (kernel, label, n, len(rl), ', '.join('%s[%s]' % (r[1], r[2]) for r in rl)))
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('listing')
    ap.add_argument('kernel')
    ap.add_argument('--loop-at', action='append', default=[], metavar='FILE:LINE')
    ap.add_argument('--loop-with', action='append', default=[], metavar='MNEMONIC,...',
                    help='the smallest loop holding all of these mnemonics (prefixes), e.g. v_exp_f32,s_ff1_i32_b64*8')
    ap.add_argument('--step-loops', action='store_true', help="the step kernel's fast reception round loop and PF leader-run loop")
    ap.add_argument('--sites', action='store_true', help='list every reload with its lane, depth and source line')
    a = ap.parse_args()
    res = analyse(a.listing, a.kernel)
    enc = res['enclosing']
    print('%s: %d instructions, %d loops, spill VGPRs %s' % (res['name'], len(res['insts']), len(res['spans']), ' '.join(res['spill_regs']) or '-'))
    by_depth, st_depth = {}, {}
    for r in res['reloads']:
        by_depth[len(enc(r[0]))] = by_depth.get(len(enc(r[0])), 0) + 1
    for s in res['stores']:
        st_depth[len(enc(s[0]))] = st_depth.get(len(enc(s[0])), 0) + 1
    print('spill stores (v_writelane): %d, by loop depth %s' % (len(res['stores']), dict(sorted(st_depth.items()))))
    print('spill reloads (v_readlane): %d, by loop depth %s' % (len(res['reloads']), dict(sorted(by_depth.items()))))
    nvalu = sum(1 for mn, _, _ in res['insts'] if mn.startswith('v_'))
    print('VALU instructions (static): %d, s_nop: %d' % (nvalu, sum(1 for mn, _, _ in res['insts'] if mn == 's_nop')))
    bad = 0
    for spec in a.loop_at:
        fname, line = spec.rsplit(':', 1)
        span = innermost_loop_at(res, fname, int(line))
        if span is None:
            print('%s: no loop holds an instruction of that line' % spec)
            bad += 1
            continue
        rl = reloads_in(res, span)
        print('%s: innermost loop of %d instructions at depth %d, %d spill reloads%s' % (
            spec, span[1] - span[0] + 1, len(enc(span[0])), len(rl),
            (' (' + ', '.join('%s[%s] %s:%s' % (r[1], r[2], r[3][0], r[3][1]) for r in rl) + ')') if rl else ''))
    named = [(spec, spec) for spec in a.loop_with] + (list(STEP_LOOPS.items()) if a.step_loops else [])
    for label, spec in named:
        span = innermost_loop_with(res, spec.split(','))
        if span is None:
            print('%s: no loop fits' % label)
            bad += 1
            continue
        rl = reloads_in(res, span)
        if a.step_loops and label in STEP_LOOPS and rl:
            bad += 1   # --step-loops is a check: a reload in either loop fails it
        print('%s: smallest loop of %d instructions at depth %d, %d spill reloads%s' % (
            label, span[1] - span[0] + 1, len(enc(span[0])), len(rl), (' (' + ', '.join('%s[%s]' % (r[1], r[2]) for r in rl) + ')') if rl else ''))
    if a.sites:
        for r in res['reloads']:
            print('  reload %s[%s] depth %d  %s:%s' % (r[1], r[2], len(enc(r[0])), r[3][0], r[3][1]))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
