"""Kernel set and resources of two device assemblies of one source file (hipcc ... --cuda-device-only -S), kernel by kernel: the
.amdhsa_kernel descriptor (next_free_vgpr, next_free_sgpr, accum_offset, group_segment_fixed_size, private_segment_fixed_size), the
occupancy comment of the kernel and the instruction text between its label and its .Lfunc_end, comments dropped and the function
ordinal of block labels (.LBB<ordinal>_<n>) normalised.  The method of profiles/r23_nt_routes.md as a tool.

    python profiles/probes/kernel_diff.py parent.s new.s [name-filter]
"""
import re
import sys

KEYS = ('next_free_vgpr', 'next_free_sgpr', 'accum_offset', 'group_segment_fixed_size', 'private_segment_fixed_size')


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', text, re.S):
        name, desc = m.group(1), m.group(2)
        res = {k: int(re.search(r'\.amdhsa_%s (\d+)' % k, desc).group(1)) for k in KEYS}
        body = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:' % re.escape(name), text, re.S | re.M).group(1)
        occ = re.search(r'; Occupancy: (\d+)', text[m.end():])
        res['occupancy'] = int(occ.group(1)) if occ else -1
        lines = [re.sub(r'\s*;.*$', '', l).strip() for l in body.split('\n')]
        lines = [re.sub(r'\.LBB\d+_', '.LBB_', l) for l in lines if l]
        out[name] = (res, lines)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pat = sys.argv[3] if len(sys.argv) > 3 else ''
    names = sorted(n for n in set(a) | set(b) if pat in n)
    gone, added = [n for n in names if n not in b], [n for n in names if n not in a]
    res_diff = [n for n in names if n in a and n in b and a[n][0] != b[n][0]]
    text_diff = [n for n in names if n in a and n in b and a[n][1] != b[n][1]]
    print('kernels: %d -> %d, gone %d, added %d, resource figures differ %d, instruction text differs %d'
          % (len([n for n in names if n in a]), len([n for n in names if n in b]), len(gone), len(added), len(res_diff), len(text_diff)))
    for n in gone:
        print('gone   ', n)
    for n in added:
        print('added  ', n)
    for n in res_diff:
        print('figures', n, a[n][0], '->', b[n][0])
    for n in text_diff:
        print('text   ', n, '%d -> %d instructions' % (len(a[n][1]), len(b[n][1])))
    if '-v' in sys.argv:
        for n in names:
            if n in b:
                print(n, ' '.join('%s=%d' % kv for kv in b[n][0].items()))


if __name__ == '__main__':
    main()
