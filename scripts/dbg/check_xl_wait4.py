"""Check the x_dma waits of the four-row-tile passes (route_fwd32_kernel /
route_bwd32_kernel <32,32,NW,4>) against their ISA.  There the DMA of capsule i + 2 is
issued after capsule i's barrier and waited for (xl_wait) before capsule i + 1's, so the
walk from each global_load_lds of the capsule loop (the innermost loop, inside the
workgroup's segment loop) to the next s_barrier wraps around the loop's back edge: the
last 's_waitcnt vmcnt(K)' on that walk must leave at most as many vector-memory
operations in flight as the wave issued after the DMA.
    python scripts/dbg/check_xl_wait4.py ISA.s"""
import re
import sys

s = open(sys.argv[1]).read()
bad = 0
for name in re.findall(r'^(_Z\w*route_(?:fwd|bwd)32_kernelILi32ELi32ELi[248]ELi4E\w*):', s, re.M):
    body = s[s.index(name + ':'):]
    body = body[:body.index('.Lfunc_end')]
    raw = body.split('\n')
    # the capsule loop: the innermost one (inside the segment loop of the workgroup); its
    # label stands on the header comment's line or on a line before it
    hdr = [k for k, l in enumerate(raw) if 'Inner Loop Header' in l][:1]
    while not re.match(r'\.LBB\d+_\d+:', raw[hdr[0]]):
        hdr[0] -= 1
    lab = raw[hdr[0]].split(':')[0]
    # the loop's blocks in layout order: the header's and every block the compiler marks
    # 'in Loop: Header=<it>'.  A latch block laid out ahead of the header (it falls through
    # into it; the loop is entered by a branch to the header) belongs to the loop as well,
    # and the cyclic walk below takes the blocks in the order they run.
    mark = 'Header=' + lab.lstrip('.L') + ' '
    lines, inloop = [], False
    for l in raw:
        if re.match(r'(\.LBB\d+_\d+:|; %bb\.\d+:)', l):
            inloop = l.startswith(lab + ':') or mark in l
        elif inloop and l.startswith('\t') and not l.strip().startswith(';'):
            lines.append(l.strip())
    for k, l in enumerate(lines):
        if not l.startswith('global_load_lds'):
            continue
        n, last = 0, None
        for step in range(1, len(lines)):
            l2 = lines[(k + step) % len(lines)]
            m = re.match(r's_waitcnt vmcnt\((\d+)\)$', l2)
            if m:
                last = (n, int(m.group(1)))
            if l2.startswith('s_barrier'):
                break
            if re.match(r'(buffer|global)_(load|store|atomic)', l2) and not l2.startswith('global_load_lds'):
                n += 1
        tag = f'{name[:70]} dma@{k}'
        if last is None:
            print(f'{tag}: no wait before the barrier')
            bad += 1
        elif last[1] > last[0]:
            print(f'{tag}: vmcnt({last[1]}) with {last[0]} operations after the DMA: TOO FEW')
            bad += 1
        else:
            print(f'{tag}: vmcnt({last[1]}), {last[0]} operations after the DMA: ok')
sys.exit(1 if bad else 0)
