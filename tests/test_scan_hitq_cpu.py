"""The queued arrangement of the int8 tile's filter (ScanCfg::FILT = 2; no GPU needed): register budget and LDS size of every k_scan
instantiation of the int8 tile that either library launches -- the measurement ones (INSTR) included --, the instantiation sets, and
the dbg-only switch that puts a pass on the queue (AK_SCAN_HITQ).

A pass takes its arrangement from its tile type (FILT the main pass, FILT_SEED the seeding pass). CfgP8 is what ships: the main pass
on the whole-tile filter, the seeding pass on the queue. CfgP8f (site by site on both) and CfgP8g (main pass queued, seeding pass
whole tile) hold the other arrangements, in the dbg library, which instantiates all three for both passes, each with and without the
counters."""
import os
import re
import subprocess

import pytest

from scripts.kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_PLAN_H = os.path.join(ROOT, "archi_amd", "csrc", "scan_plan.h")      # the tile types: constants and static_asserts only
P8 = re.compile(r"void ak::k_scan<true, ak::(CfgP8[fg]?), false, (true|false), (true|false)>")


def _const(name):
    m = re.search(rf"\b{name} = (\d+)\b", open(SCAN_PLAN_H).read())
    assert m, name
    return int(m.group(1))


TYPES = ("CfgP8", "CfgP8f", "CfgP8g")


def _p8_kernels(extra_flags):
    """{(type, INSTR, SEEDPASS): resources} of the int8 tile's k_scan instantiations of one build."""
    res = kernel_resources("scan.hip", extra_flags=extra_flags)
    names = subprocess.run(["c++filt"] + list(res), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    out = {}
    for (_, r), name in zip(res.items(), names):
        m = P8.match(name)
        if m:
            out[(m.group(1), m.group(2) == "true", m.group(3) == "true")] = r
    return out


@pytest.mark.parametrize("library,flags", [("product", []), ("dbg", ["-DAK_DBG_KERNELS=1"])])
def test_no_int8_scan_kernel_spills_and_the_queued_ones_exist_where_they_are_launched(library, flags):
    got = _p8_kernels(flags)
    for key, r in got.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] <= 8, (library, key, r)
    if library == "dbg":
        # every arrangement of either pass, production and measurement instantiation: the queued ones are CfgP8's seeding pass and
        # CfgP8g's main pass
        assert set(got) == {(t, i, s) for t in TYPES for i in (False, True) for s in (False, True)}, sorted(got)
    else:
        assert set(got) == {("CfgP8", False, False), ("CfgP8", False, True)}, sorted(got)      # no other type, no counters
    # what ships: the main pass on the whole tile, the seeding pass on the queue
    assert _const("SHIP_FILT_P8") == 1 and _const("SHIP_FILT_P8_SEED") == 2


def test_the_queued_tile_fits_the_lds():
    """The queues lie behind the common layout of the 256 x 256 tile: two K-tile buffers of A and B (128 B per row), the per-row terms,
    thresholds, counts, margins and triggers, the request word and the block bounds -- 139 792 bytes -- plus [8 waves][HQ_WORDS][HQ_SLOTS]
    words. The compiler holds ScanCfg to the same figure (static_assert `LDS budget`); the kernels' LDS is dynamic, so the resource
    remark does not show it."""
    src = open(SCAN_PLAN_H).read()
    words, slots = _const("HQ_WORDS"), _const("HQ_SLOTS")
    assert words == 9 and slots == 64                                   # eight dot products + (site, lane); one slot per lane of the drain
    common = 2 * (256 * 128 + 256 * 128) + (4 * 256 + 4 * 256 + 4 + 128) * 4
    assert common == 139792
    assert common + 8 * words * slots * 4 <= 160 * 1024
    assert re.search(r"static_assert\(SEED_LDS_BYTES <= 160 \* 1024 && LDS_BYTES <= 160 \* 1024", src)
    assert "HQ_BYTES = (FM == 2 || FS == 2) ? Base::NW * Base::HQ_WORDS * Base::HQ_SLOTS * 4 : 0" in src
    assert 'static_assert(LDS_BYTES <= 160 * 1024, "LDS budget")' in src


def test_the_product_library_refuses_the_queue_switch():
    import __graft_entry__ as ge
    ge.build()
    from archi_amd import _lib
    set_switch = _lib.load().ak_debug_set
    assert all(set_switch(b"AK_SCAN_HITQ", str(v).encode()) != 0 for v in (1, 2, 3, 4, 5, -1))
    assert set_switch(b"AK_SCAN_HITQ", b"0") == 0 and set_switch(b"AK_SCAN_HITQ", None) == 0
