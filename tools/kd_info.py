"""Register / LDS / scratch figures of kernels in libvio360.so builds (code-object metadata, CPU only).
usage: python tools/kd_info.py <lib.so> [<lib.so> ...] [--match substr]
code_objects(lib) is also what tools/isa_mix.py reads a library through."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import test_build as tb  # noqa: E402


def code_objects(lib):
    """[(gfx950 code object bytes, {kernel name: its amdhsa.kernels metadata entry})] of a library"""
    blob = open(lib, "rb").read()
    return [(co, {kd[".name"]: kd for kd in tb._kernel_descriptors(co)}) for co in tb._gfx950_code_objects(blob)]


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    match = next((a.split("=", 1)[1] for a in argv if a.startswith("--match=")), "ph_")
    for lib in args:
        print("==", lib)
        for _, kds in code_objects(lib):
            for name, kd in kds.items():
                if match in name:
                    print(f"  {name[:70]:70s} vgpr={kd['.vgpr_count']:4d} agpr={kd.get('.agpr_count', 0):3d} "
                          f"sgpr={kd['.sgpr_count']:3d} lds={kd['.group_segment_fixed_size']:6d} "
                          f"scratch={kd['.private_segment_fixed_size']:4d} spill_v={kd.get('.vgpr_spill_count', 0)}")


if __name__ == "__main__":
    main(sys.argv[1:])
