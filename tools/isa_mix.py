"""Static instruction mix of gfx950 kernels (CPU only): counts by class from the disassembly of the code
objects in a libvio360.so build, or from one .hip file compiled to assembly, plus the VGPR / LDS / private
segment figures of the code-object metadata (read through tools/kd_info.py).
Classification is by mnemonic prefix only; the counts are static (every instruction once, whatever a loop
or a branch does with it).
usage: python tools/isa_mix.py <lib.so | file.hip> [--match=substr] [--sections] [-- extra hipcc flags]
  --sections   also print the mix of each stretch between two s_barrier instructions
  int_div      expansions of a runtime integer division or remainder (one v_rcp_iflag_f32 each)"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kd_info  # noqa: E402

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "360_visual_inertial_odometry_amd", "csrc")
CLASSES = ("valu", "f64", "mov", "sel_cmp", "salu", "lds", "vmem", "smem", "barrier", "int_div", "other")
_F64 = re.compile(r"^v_\w+_f64|^v_cvt_\w*f64|^v_mfma_f64")
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")


def classify(m):
    """classes of one mnemonic: its issue class, and for VALU the sub-classes it also counts under"""
    if m == "s_barrier":
        return ("barrier",)
    if m.startswith(("s_load", "s_buffer_load")):
        return ("smem",)
    if m.startswith("s_"):
        return ("salu",)
    if m.startswith("ds_"):
        return ("lds",)
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return ("vmem",)
    if m.startswith("v_"):
        out = ["valu"]
        if m.startswith("v_rcp_iflag"):
            out.append("int_div")
        if m.startswith(("v_mov_", "v_accvgpr_", "v_readlane", "v_readfirstlane", "v_writelane")):
            out.append("mov")
        elif m.startswith(("v_cndmask", "v_cmp", "v_cmpx")):
            out.append("sel_cmp")
        elif _F64.match(m) and not m.startswith("v_cmp"):
            out.append("f64")
        return tuple(out)
    return ("other",)


def functions(text):
    """(name, [mnemonic, ...]) of every function of an assembly listing or an llvm-objdump disassembly"""
    name, ins = None, []
    for line in text.splitlines():
        lab = re.match(r"^(?:[0-9a-f]+ <)?([A-Za-z_][\w$.]*)>?:\s*(?:;.*|//.*)?$", line)
        if lab and not lab.group(1).startswith((".L", "L", "BB")):
            if name and ins:
                yield name, ins
            name, ins = lab.group(1), []
            continue
        if line.lstrip().startswith((".", ";", "//")) or name is None:
            if ".end_amdhsa_kernel" in line or ".Lfunc_end" in line:
                if name and ins:
                    yield name, ins
                name, ins = None, []
            continue
        m = _INSN.match(line)
        if m:
            ins.append(m.group(1))
    if name and ins:
        yield name, ins


def mix(ins):
    c = collections.Counter()
    for m in ins:
        for k in classify(m):
            c[k] += 1
    return c


def fmt(c):
    return " ".join(f"{k}={c[k]}" for k in CLASSES if c[k] or k in ("valu", "f64", "int_div"))


def report(name, ins, kd, sections):
    print(name)
    if kd:
        print(f"  vgpr={kd['.vgpr_count']} agpr={kd.get('.agpr_count', 0)} sgpr={kd['.sgpr_count']} "
              f"lds={kd['.group_segment_fixed_size']} private={kd['.private_segment_fixed_size']}")
    print("  total  " + fmt(mix(ins)))
    if sections:
        part, n = [], 0
        for m in ins + ["s_barrier"]:
            part.append(m)
            if m == "s_barrier":
                print(f"  sec{n:<3d} " + fmt(mix(part)))
                part, n = [], n + 1


def from_lib(path, match, sections):
    with tempfile.TemporaryDirectory() as tmp:
        for n, (co, kds) in enumerate(kd_info.code_objects(path)):
            if not any(match in k for k in kds):
                continue
            f = os.path.join(tmp, f"co{n}.elf")
            open(f, "wb").write(co)
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", f],
                                  check=True, capture_output=True, text=True).stdout
            for name, ins in functions(text):
                if match in name and name in kds:
                    report(name, ins, kds[name], sections)


def from_hip(path, match, sections, extra):
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "out.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, *extra, path, "-o", s], check=True)
        text = open(s).read()
    meta = {}
    for blk in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        g = lambda k: int((re.search(r"\.amdhsa_" + k + r" (\d+)", blk.group(2)) or [0, 0])[1])  # noqa: E731
        meta[blk.group(1)] = {".vgpr_count": g("next_free_vgpr"), ".sgpr_count": g("next_free_sgpr"),
                              ".group_segment_fixed_size": g("group_segment_fixed_size"),
                              ".private_segment_fixed_size": g("private_segment_fixed_size")}
    for name, ins in functions(text):
        if match in name and name in meta:
            report(name, ins, meta[name], sections)


def main(argv):
    extra = argv[argv.index("--") + 1:] if "--" in argv else []
    argv = argv[:argv.index("--")] if "--" in argv else argv
    match = next((a.split("=", 1)[1] for a in argv if a.startswith("--match=")), "ph_")
    sections = "--sections" in argv
    for path in [a for a in argv if not a.startswith("--")]:
        print("==", os.path.relpath(path, ROOT) if os.path.isabs(path) else path)
        if path.endswith(".hip"):
            from_hip(path, match, sections, extra)
        else:
            from_lib(path, match, sections)


if __name__ == "__main__":
    main(sys.argv[1:])
