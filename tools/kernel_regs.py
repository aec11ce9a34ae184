"""Per-kernel register / LDS / scratch use of the gfx950 code objects in libsacx.so (diagnostic):
VGPRs bound the waves per SIMD (512 / vgpr_count), hence how many workgroups of a launch
run at once.  Every offload bundle of the library is read (one per translation unit with kernels).

usage: python tools/kernel_regs.py [path/to/libsacx.so] [substring of the mangled name]
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "vgpr_spill_count")


def kernel_resources(so_path):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", so_path,
                               os.path.join(d, "copy.so")])
        blob = open(fat, "rb").read()
        # the bundler reads only the first bundle of a file: cut the section at each bundle's magic
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
            part, dev = os.path.join(d, f"fat{i}.bin"), os.path.join(d, f"dev{i}.o")
            with open(part, "wb") as fh:
                fh.write(blob[a:b])
            subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={dev}"])
            notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", dev], text=True)
            # one YAML list item per kernel ("  - .agpr_count: ..."); keys before and after .name belong to it
            cur = None
            for line in notes.splitlines():
                if re.match(r"\s{2}- \.", line):
                    cur = {}
                if cur is None:
                    continue
                m = re.match(r"\s*-?\s*\.name:\s+(\S+)", line)
                if m:
                    out[m.group(1)] = cur
                for key in KEYS:
                    m = re.match(r"\s*-?\s*\.%s:\s+(\d+)" % key, line)
                    if m:
                        cur[key] = int(m.group(1))
    return out


def main():
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "sac-expert_amd", "lib", "libsacx.so")
    pat = sys.argv[2] if len(sys.argv) > 2 else ""
    for n, v in sorted(kernel_resources(so).items()):
        if pat in n:
            vg = v.get("vgpr_count", 0)
            print(f"{n:70s} vgpr {vg:4d} agpr {v.get('agpr_count', 0):3d} sgpr {v.get('sgpr_count', 0):3d} "
                  f"lds {v.get('group_segment_fixed_size', 0):6d} scratch {v.get('private_segment_fixed_size', 0):4d}"
                  f"  waves/SIMD {min(8, 512 // max(vg, 1))}")


if __name__ == "__main__":
    main()
