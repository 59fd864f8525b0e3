"""Per-kernel resource usage of one .hip file of archi_amd/csrc, compiled for gfx950 with the Makefile's FLAGS and
-Rpass-analysis=kernel-resource-usage (no GPU needed).

    from scripts.kernel_resources import kernel_resources
    kernel_resources("mbert.hip") -> {mangled kernel name: {"VGPRs": .., "AGPRs": .., "VGPRs Spill": .., "SGPRs Spill": ..,
                                      "ScratchSize [bytes/lane]": .., "LDS Size [bytes/block]": .., "Occupancy [waves/SIMD]": .., ...}}

    python scripts/kernel_resources.py scan.hip [filter]      one line per kernel, demangled names
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "archi_amd", "csrc")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


def makefile_flags():
    """FLAGS of archi_amd/csrc/Makefile, $(ARCH) expanded."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*:=\s*(\S+)", mk, re.M).group(1)
    return re.search(r"^FLAGS\s*:=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()


def kernel_resources(src, csrc=CSRC, extra_flags=()):
    """src: a file name in `csrc` (or a path) -> {kernel: {field: value}}; every integer field of the compiler's remark, under the
    compiler's names. extra_flags: on top of the Makefile's, e.g. ["-DAK_DBG_KERNELS=1"] for the dbg library's instantiations.
    Raises RuntimeError with the compiler's output when the file does not compile."""
    r = subprocess.run([HIPCC] + makefile_flags() + list(extra_flags) + ["--cuda-device-only", "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage",
                                                     os.path.join(csrc, src)], capture_output=True, text=True, cwd=csrc)
    if r.returncode:
        raise RuntimeError(f"{src}: hipcc failed\n{r.stderr[-4000:]}")
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        key, _, value = m.group(1).strip().partition(":")
        if key == "Function Name":
            cur = out.setdefault(value.strip(), {})
        elif cur is not None and re.fullmatch(r"\s*\d+", value):
            cur[key.strip()] = int(value)
    return out


def main():
    src, flt = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""
    try:
        res = kernel_resources(src)
    except RuntimeError as e:
        print(e)
        sys.exit(1)
    names = subprocess.run(["c++filt"] + list(res), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    for (_, r), n in zip(res.items(), names):
        n = re.sub(r"\(.*", "", n)
        if flt and flt not in n:
            continue
        print(f"{n[:110]:110s} vgpr {r.get('VGPRs', '?'):>3} agpr {r.get('AGPRs', '?'):>3} vspill {r.get('VGPRs Spill', '?'):>3} "
              f"scratch {r.get('ScratchSize [bytes/lane]', '?'):>4} sgpr {r.get('TotalSGPRs', '?'):>3} sspill {r.get('SGPRs Spill', '?'):>3} "
              f"lds {r.get('LDS Size [bytes/block]', '?'):>5} occ {r.get('Occupancy [waves/SIMD]', '?')}")


if __name__ == "__main__":
    main()
