"""Register table of the gradient instantiations of the Rys quartet kernels, from code-object metadata alone.
usage: python tools/grad_kernel_registers.py grad.o [grad_before.o] [out.txt]        (CPU only)

Unbundles the gfx950 code object of a compiled csrc/grad.hip (dqc_amd/csrc/_obj/grad.o after a build) and reads, for every
eri_kernel<LA, LB, LC, LD, MODE> and eri_hl_kernel<TPQ, MODE> in it, the VGPR count, SGPR count and private-segment size from the
AMDGPU metadata note.  With a second object (the same source compiled at another commit) the ERI_OUT_GRAD rows (MODE 3) of the two are
compared and the differing ones listed; the ERI_OUT_GRAD3 rows (MODE 7) are listed beside the ERI_OUT_GRAD row of the same class."""
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
        if mode not in (3, 7):
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
    objs = [a for a in args if a.endswith(".o")]
    outs = [a for a in args if not a.endswith(".o")]
    now = kernels(objs[0])
    lines = []
    grad = sorted(k for k in now if with_mode(k, 3) == k)
    if len(objs) > 1:
        before = kernels(objs[1])
        gb = sorted(k for k in before if with_mode(k, 3) == k)
        changed = [k for k in grad if before.get(k) != now[k]] + [k for k in gb if k not in now]
        lines.append("ERI_OUT_GRAD instantiations: %d before, %d now, %d differ in (vgpr, sgpr, private segment)" % (len(gb), len(grad), len(changed)))
        for k in changed:
            lines.append("  DIFFERS %-12s before %s now %s" % (label(k), before.get(k), now.get(k)))
    lines.append("%-12s %-20s %-20s" % ("class", "GRAD vgpr/sgpr/priv", "GRAD3 vgpr/sgpr/priv"))
    for k in grad:
        k3 = with_mode(k, 7)
        lines.append("%-12s %-20s %-20s" % (label(k), "%d / %d / %d" % now[k], "%d / %d / %d" % now[k3] if k3 in now else "-"))
    txt = "\n".join(lines)
    print(txt)
    if outs:
        open(outs[0], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
