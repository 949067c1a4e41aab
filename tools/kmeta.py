"""Print per-kernel resource usage (VGPRs, spills, SGPRs, scratch, LDS) and the MFMA / LDS-DMA instruction counts from a hipcc .s file."""
import re
import sys

s = open(sys.argv[1]).read()
md = s[s.index("amdhsa.kernels:"):]


def count(name, pat):      # instructions matching pat between the kernel's label and the end of its function
    m = re.search(r"^%s:.*?^\.Lfunc_end" % re.escape(name), s, re.S | re.M)
    return len(re.findall(pat, m.group(0), re.M)) if m else -1


for blk in md.split("  - .agpr_count:")[1:]:
    def g(k):
        m = re.search(re.escape(k) + r":\s+(\S+)", blk)
        return m.group(1) if m else "?"
    print("%-72s vgpr %4s agpr %4s spill %3s sgpr %4s scratch %4s lds %s mfma %d ldsdma %d" % (
        g(".name")[:72], g(".vgpr_count"), blk.split()[0], g(".vgpr_spill_count"), g(".sgpr_count"),
        g(".private_segment_fixed_size"), g(".group_segment_fixed_size"),
        count(g(".name"), r"^\s+v_mfma"), count(g(".name"), r"^\s+buffer_load.* lds$")))
