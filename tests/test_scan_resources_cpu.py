"""Register budget of the scan kernels, from the compiler's own resource remarks (no GPU needed). The 256 x 256 phased tile runs
at the edge of the 256-register file -- 128 accumulators, 64 fragment registers, the staging offsets -- and a change that tips
it into spilling turns the MFMA-bound K-loop into a scratch-bound one without failing any result test."""
import re
import subprocess

from scripts.kernel_resources import kernel_resources

# ScratchSize of the filtering k_scan kernels before the 16x16x32 variant was added: 8 bytes per lane (the frame of the
# out-of-line compaction routine), none in the pre-seeding kernels. No variant may need more.
PARENT_SCRATCH_BYTES_PER_LANE = 8


def test_no_scan_kernel_spills_vector_registers_or_grows_its_scratch():
    res = kernel_resources("scan.hip")
    names = subprocess.run(["c++filt"] + list(res), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    checked, shapes = 0, set()
    for (_, r), name in zip(res.items(), names):
        m = re.match(r"void ak::k_scan<(true|false), ak::ScanCfg<([^>]*)>, (true|false), (true|false), (true|false)>", name)
        if not m:
            continue
        if m.group(4) == "true":          # INSTR: the measurement instantiation (dbg library only)
            continue
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] <= PARENT_SCRATCH_BYTES_PER_LANE, (name, r)
        checked += 1
        shapes.add(m.group(2).split(", ")[-1])
    assert checked >= 24, checked          # 6 tiles x 2 dtypes x (pre-seeding, seeding pass, main pass) at least
    assert "32" in shapes                  # the shape parameter is where this test reads it
