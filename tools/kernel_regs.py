"""Register / spill / LDS use of the render kernels from device assembly.

usage: python tools/kernel_regs.py <render.s> [name-regex]   (hipcc ... --cuda-device-only -S)

Without a regex: the render, probe and trace kernels.  With one (e.g. "atrous|guided" on
denoise.hip's assembly): the kernels whose mangled name matches it, with their LDS bytes.
"""
import re
import sys

s = open(sys.argv[1]).read()
meta = s[s.index("amdhsa.kernels:"):]
for blk in meta.split("  - .agpr_count")[1:]:
    name = re.search(r"\.name:\s+(\S+)", blk).group(1)
    if len(sys.argv) > 2:
        if not re.search(sys.argv[2], name):
            continue
    elif "render_kernel" not in name and "probe" not in name and "trace_kernel" not in name:
        continue
    g = lambda k: (re.search(r"\.%s:\s+(\d+)" % k, blk) or [None, None])[1]
    print(f"{name[:70]:70s} vgpr {g('vgpr_count')} spill {g('vgpr_spill_count')} sgpr {g('sgpr_count')} "
          f"sspill {g('sgpr_spill_count')} private {g('private_segment_fixed_size')}"
          + (f" lds {g('group_segment_fixed_size')}" if len(sys.argv) > 2 else ""))
