#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device assemblies of one source (another commit's against this tree's), for changes
that are meant to leave the device code alone: instruction count, next_free_vgpr, accum_offset, next_free_sgpr, LDS and
private-segment bytes, wavefronts per SIMD by registers (512 per lane, granule 8), and for every kernel whose instruction
histogram moved the opcodes that moved.  Exit status 1 if LDS bytes differ, the private segment grew, a kernel lost a
wavefront per SIMD, or a kernel whose name matches --unchanged REGEX (the kernels a change must not touch at all) differs in
its histogram or in any column.  Whether a moved histogram is acceptable is not this tool's to say: read the list.
The assemblies come from (flags: se3conv3d_amd/build.py FLAGS)

    hipcc <FLAGS> --cuda-device-only -S se3conv3d_amd/csrc/edge_bf16.hip -o this.s
    usage: tools/isa_diff.py [--unchanged REGEX] parent.s this.s"""
import collections, re, subprocess, sys


def parse(path):
    hist, meta, name, hsa = {}, collections.defaultdict(dict), None, None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            hist[name] = collections.Counter()
        elif s.startswith(".Lfunc_end"):  # (not s_endpgm: the exit block may be laid out in front of the loop body)
            name = None
        elif s.startswith(".amdhsa_kernel "):
            hsa = s.split()[1]
        elif s.startswith(".end_amdhsa_kernel"):
            hsa = None
        elif hsa and s.startswith(".amdhsa_"):
            key, _, val = s.partition(" ")
            meta[hsa][key[len(".amdhsa_"):]] = val.strip()
        elif name and line.startswith("\t") and s and s[0] not in ".;":
            hist[name][s.split()[0]] += 1
    return hist, meta


def waves(vgpr):
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


def main():
    args, keep = sys.argv[1:], None
    if args and args[0] == "--unchanged":
        keep, args = re.compile(args[1]), args[2:]
    (ph, pm), (th, tm) = parse(args[0]), parse(args[1])
    names = sorted(set(pm) | set(tm))
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    cols = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")
    print(f"{'kernel (parent / this tree)':60s} {'instructions':>13s} {'vgpr':>9s} {'accum':>9s} {'sgpr':>9s} {'LDS':>15s} {'private':>9s} {'w/SIMD':>6s}")
    bad, moved = 0, []
    for n, full in zip(names, plain):
        if n not in pm or n not in tm:
            print(f"{full}: only in {'the parent' if n in pm else 'this tree'}")
            bad += 1
            continue
        short = re.sub(r"^(void )?se3::(\(anonymous namespace\)::)?", "", full).split("(")[0]
        p = [sum(ph[n].values())] + [int(pm[n].get(c, 0)) for c in cols]
        t = [sum(th[n].values())] + [int(tm[n].get(c, 0)) for c in cols]
        flags = []
        if p[4] != t[4]: flags.append("LDS differs")
        if t[5] > p[5]: flags.append("private segment grew")
        if waves(t[1]) < waves(p[1]): flags.append("lost a wavefront per SIMD")
        if keep and keep.search(short) and (p != t or ph[n] != th[n]): flags.append("must be unchanged")
        bad += bool(flags)
        if ph[n] != th[n]:
            flags.append("histogram moved")
            moved.append((short, {op: th[n][op] - ph[n][op] for op in set(ph[n]) | set(th[n]) if th[n][op] != ph[n][op]}))
        print(f"{short[:60]:60s} {p[0]:6d}/{t[0]:6d} {p[1]:4d}/{t[1]:4d} {p[2]:4d}/{t[2]:4d} {p[3]:4d}/{t[3]:4d} {p[4]:7d}/{t[4]:7d} {p[5]:4d}/{t[5]:4d} "
              f"{waves(p[1]):3d}/{waves(t[1]):d}  {', '.join(flags)}")
    print()
    for short, d in moved:
        print(f"moved: {short}: " + " ".join(f"{op}{v:+d}" for op, v in sorted(d.items())))
    print(f"kernels: {len(names)}, histogram moved: {len(moved)}, conditions violated: {bad}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
