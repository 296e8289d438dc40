#!/usr/bin/env python3
"""Registers, LDS, scratch and code bytes of every kernel of one source file at two commits, side by side, and the offline
facts about the staged kernels' prologue, staging rounds and seed scan (profiles/prologue_kernel_resources.txt).  No GPU.
usage: tools/kernel_resources_ab.py <parent.s> <head.s>
where each .s is the gfx950 device assembly of csrc/scg_kernels.hip at that commit:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-pass-failed -Iinclude -Iscreencounter_amd/csrc --save-temps \
        --cuda-device-only -c screencounter_amd/csrc/scg_kernels.hip      (writes scg_kernels-hip-amdgcn-amd-amdhsa-gfx950.s)
"""
import re, sys

def kernels(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'- \.agpr_count:.*?\.wavefront_size', s, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r'\.%s:\s+(\S+)' % k, blk).group(1)
        out[g('name')] = dict(vgpr=int(g('vgpr_count')), sgpr=int(g('sgpr_count')), lds=int(g('group_segment_fixed_size')), scratch=int(g('private_segment_fixed_size')))
    for m in re.finditer(r'^(_Z\w+):.*?; codeLenInByte = (\d+)', s, re.S | re.M):
        if m.group(1) in out and 'code' not in out[m.group(1)]:
            out[m.group(1)]['code'] = int(m.group(2))
    return out, s

def body(s, name):
    a = s.index('\n' + name + ':')
    b = s.index('.Lfunc_end', a)
    return [l.strip() for l in s[a:b].split('\n') if l.startswith('\t') and not l.strip().startswith(('.', ';'))]

def waves(v):
    return min(8, 512 // (-(-v // 8) * 8))

def facts(s, name):
    ins = body(s, name)
    first_ld = next(i for i, l in enumerate(ins) if l.startswith('global_load_dwordx4') and ' nt' in l)
    first_st = next(i for i, l in enumerate(ins) if l.startswith('ds_write_b32') or l.startswith('ds_write_b128'))
    nt = [i for i, l in enumerate(ins) if l.startswith('global_load_dwordx4') and ' nt' in l]
    counted = sorted({l for l in ins if re.match(r's_waitcnt vmcnt\([1-9]\)', l)})
    smem = sum(1 for l in ins if l.startswith('s_load'))
    # the compact seed scan: the stretches of funnel shifts by a scalar register (the walk words), and the scalar loads inside them
    scal = [i for i, l in enumerate(ins) if re.match(r'v_alignbit_b32 v\d+, v\d+, v\d+, s\d+', l)]
    inside = 0
    if scal:
        # per seed loop body: count scalar loads strictly between consecutive scalar-shift instructions that are < 40 instructions apart
        for a, b in zip(scal, scal[1:]):
            if b - a < 40:
                inside += sum(1 for l in ins[a:b] if l.startswith('s_load'))
    return dict(instructions=len(ins), first_nt_load=first_ld, first_table_store=first_st, nt_loads=len(nt), counted_waits=counted, s_loads=smem,
                s_loads_inside_walk_shifts=inside, writelane=sum(1 for l in ins if l.startswith('v_writelane')))

P, ps = kernels(sys.argv[1])
H, hs = kernels(sys.argv[2])
print("# kernel (mangled, first 100 characters)                                                               | parent: vgpr sgpr lds scratch code waves wg/CU | head: vgpr sgpr lds scratch code waves wg/CU | note")
changed = 0
for name in H:
    h, p = H[name], P.get(name)
    def col(k):
        w = waves(k['vgpr']); wg = min(w, 163840 // k['lds']) if k['lds'] else w
        return "%4d %4d %6d %4d %6d %2d %2d" % (k['vgpr'], k['sgpr'], k['lds'], k['scratch'], k.get('code', 0), w, wg)
    note = ""
    if p:
        if h['scratch'] > p['scratch']: note = "SCRATCH GREW"
        elif h['scratch'] < p['scratch']: note = "scratch shrank"
        if h['lds'] > p['lds']: note += " LDS GREW"
        if waves(h['vgpr']) < waves(p['vgpr']): note += " FEWER WAVES"
        if waves(h['vgpr']) > waves(p['vgpr']): note += " more waves"
        if (h['vgpr'], h['sgpr'], h['scratch'], h.get('code')) != (p['vgpr'], p['sgpr'], p['scratch'], p.get('code')): changed += 1
    print("%-101s | %s | %s | %s" % (name[:100], col(p) if p else "-", col(h), note.strip()))
print("# %d kernels; scratch summed over all kernels: parent %d B, head %d B; kernels whose registers, scratch or code changed: %d" % (
    len(H), sum(k['scratch'] for k in P.values()), sum(k['scratch'] for k in H.values()), changed))
print("#")
print("# Offline facts, from the same assembly (instruction indices count from the kernel's entry, in program-text order):")
for pat in ('single_staged_kernelILi5ELi2ELi3Ej', 'combo_staged_kernelILi5ELi2ELi3ELb0Ej'):
    name = [n for n in H if re.search(pat, n)][0]
    for tag, s in (("parent", ps), ("head", hs)):
        f = facts(s, name)
        print("# %-6s %s" % (tag, name[:70]))
        print("#        first non-temporal 16-byte load at instruction %d, first strand-table store at %d; %d such loads in the kernel" % (f['first_nt_load'], f['first_table_store'], f['nt_loads']))
        print("#        counted vmcnt waits: %s" % (", ".join(f['counted_waits']) or "none (vmcnt(0) only)"))
        print("#        scalar loads: %d in the kernel, %d between two funnel shifts of a seed walk; v_writelane (SGPR spills) %d; %d instructions" % (
            f['s_loads'], f['s_loads_inside_walk_shifts'], f['writelane'], f['instructions']))
