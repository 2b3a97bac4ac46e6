"""Register table of the gradient instantiations of the Rys quartet kernels, from code-object metadata alone.
usage: python tools/grad_kernel_registers.py grad.o [grad_before.o] [grad2.o] [out.txt]        (CPU only)

Unbundles the gfx950 code object of a compiled csrc/grad.hip (dqc_amd/csrc/_obj/grad.o after a build) and reads, for every
eri_kernel<LA, LB, LC, LD, MODE> and eri_hl_kernel<TPQ, MODE> in it, the VGPR count, SGPR count and private-segment size from the
AMDGPU metadata note.  With a second object (the same source compiled at another commit) the ERI_OUT_GRAD rows (MODE 3) of the two are
compared and the differing ones listed, and so are the ERI_OUT_GRAD3 rows (MODE 7); those are listed beside the ERI_OUT_GRAD row of the
same class, with the ERI_OUT_GRAD2 rows (MODE 8) of csrc/grad2.hip when its object (a file named grad2*.o) is given too."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def kernels(obj):
    """{(kernel, template arguments): (vgpr, sgpr, private segment bytes)} of the gradient modes in `obj`"""
    d = tempfile.mkdtemp(prefix="regs_")
    fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "gfx950.co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(d, "unused.o")], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--output=" + co,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for e in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        m = re.match(r"_ZN3dqc(?:10eri_kernel|13eri_hl_kernel)I((?:Li\d+E)+)E", name)
        if not m:
            continue
        targs = tuple(int(x) for x in re.findall(r"Li(\d+)E", m.group(1)))
        hl = "eri_hl_kernel" in name
        mode = targs[1] if hl else targs[4]
        if mode not in (3, 7, 8):
            continue
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, e).group(1))  # noqa: E731
        out[("hl" if hl else "eri", targs)] = (g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"))
    return out


def label(key):
    kind, t = key
    return "hl<tpq %d>" % t[0] if kind == "hl" else "(%d%d|%d%d)" % t[:4]


def with_mode(key, mode):
    kind, t = key
    return (kind, (t[0], mode) + t[2:]) if kind == "hl" else (kind, t[:4] + (mode,) + t[5:])


def main():
    args = sys.argv[1:]
    second = [a for a in args if a.endswith(".o") and os.path.basename(a).startswith("grad2")]
    objs = [a for a in args if a.endswith(".o") and a not in second]
    outs = [a for a in args if not a.endswith(".o")]
    now = kernels(objs[0])
    for a in second:
        now.update(kernels(a))
    lines = []
    grad = sorted(k for k in now if with_mode(k, 3) == k)
    if len(objs) > 1:
        before = kernels(objs[1])
        gb = sorted(k for k in before if with_mode(k, 3) == k)
        changed = [k for k in grad if before.get(k) != now[k]] + [k for k in gb if k not in now]
        lines.append("ERI_OUT_GRAD instantiations: %d before, %d now, %d differ in (vgpr, sgpr, private segment)" % (len(gb), len(grad), len(changed)))
        for k in changed:
            lines.append("  DIFFERS %-12s before %s now %s" % (label(k), before.get(k), now.get(k)))
        g3b = sorted(k for k in before if with_mode(k, 7) == k)
        g3n = sorted(k for k in now if with_mode(k, 7) == k)
        changed3 = [k for k in g3n if before.get(k) != now[k]] + [k for k in g3b if k not in now]
        lines.append("ERI_OUT_GRAD3 instantiations: %d before, %d now, %d differ in (vgpr, sgpr, private segment)" % (len(g3b), len(g3n), len(changed3)))
        for k in changed3:
            lines.append("  DIFFERS %-12s before %s now %s" % (label(k), before.get(k), now.get(k)))
    cell = lambda k: "%d / %d / %d" % now[k] if k in now else "-"  # noqa: E731
    priv = [k for k in grad if with_mode(k, 8) in now and now[with_mode(k, 8)][2] > 0 and now[k][2] == 0]
    lines.append("ERI_OUT_GRAD2 instantiations with a private segment where the ERI_OUT_GRAD one has none: %d%s"
                 % (len(priv), "".join(" " + label(k) for k in priv)))
    lines.append("%-12s %-20s %-20s %-20s" % ("class", "GRAD vgpr/sgpr/priv", "GRAD3 vgpr/sgpr/priv", "GRAD2 vgpr/sgpr/priv"))
    for k in grad:
        lines.append("%-12s %-20s %-20s %-20s" % (label(k), cell(k), cell(with_mode(k, 7)), cell(with_mode(k, 8))))
    txt = "\n".join(lines)
    print(txt)
    if outs:
        open(outs[0], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
