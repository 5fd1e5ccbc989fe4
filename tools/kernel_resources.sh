# per-kernel VGPR / SGPR / scratch / LDS of a built libnimble_amd.so (the
# gfx950 code objects' metadata; the library carries one offload bundle per
# kernel source file, all of them are listed): tools/kernel_resources.sh [lib]
set -e
LIB=$(realpath ${1:-nimblephysics_amd/libnimble_amd.so})
D=$(mktemp -d)
cd $D
objcopy --dump-section .hip_fatbin=fb.bin $LIB
python3 - <<'PY'
import re
import subprocess
B = "/opt/rocm/llvm/bin/"
data = open("fb.bin", "rb").read()
magic = b"__CLANG_OFFLOAD_BUNDLE__"
starts = [m.start() for m in re.finditer(magic, data)]
for i, s in enumerate(starts):
    part = f"fb{i}.bin"
    open(part, "wb").write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
    ls = subprocess.run([B + "clang-offload-bundler", "--list", "--type=o", "--input=" + part], capture_output=True,
                        text=True, check=True).stdout.split()
    tg = [t for t in ls if "gfx950" in t]
    if not tg:
        continue
    subprocess.run([B + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + tg[0], "--input=" + part,
                    f"--output=co{i}.o"], check=True)
    t = subprocess.run([B + "llvm-readelf", "--notes", f"co{i}.o"], capture_output=True, text=True, check=True).stdout
    for blk in t.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or not name.group(1).startswith("nimble_"):
            continue
        g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
        print(f"{name.group(1):44s} vgpr {g('vgpr_count'):>4s} sgpr {g('sgpr_count'):>4s} scratch {g('private_segment_fixed_size'):>6s} "
              f"vgpr_spill {g('vgpr_spill_count'):>4s} lds {g('group_segment_fixed_size')}")
PY
rm -rf $D
