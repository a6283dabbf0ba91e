"""Compiler-level budget of the fused Bottleneck kernels (no GPU): csrc/bottleneck.hip is compiled to gfx950 assembly and every
instantiated kernel must stay without scratch and spills inside 128 VGPRs (two 8-wave workgroups per CU), and the bf16 product
kernels must issue fewer plain vector instructions - neither MFMA nor transcendental - than the kernels they replaced.  The old
counts are those of the commit before the instruction diet, from profiles/bottleneck_valu.md (tools/bneck_isa_census.py)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")

# profiles/bottleneck_valu.md, "before": plain VALU instructions of the bf16 kernels, (in the code, per wave and tile)
PARENT_VALU = {"bottleneck128c_kernel": (853, 1000), "bottleneck64r_kernel": (890, 890)}


@pytest.fixture(scope="module")
def kernels():
    import bneck_isa_census as census
    res = census.census(census.compile_asm(census.SOURCE), census.SOURCE)
    return {sym: k for sym, k in res.items() if "bottleneck128c_kernel" in sym or "bottleneck64r_kernel" in sym}


def test_register_budget(kernels):
    assert len(kernels) == 4, sorted(kernels)            # two kernels x bf16 / fp16
    for name, k in kernels.items():
        meta = k["meta"]
        assert meta["private_segment_fixed_size"] == 0, name
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, name
        assert meta["vgpr_count"] <= 128, (name, meta["vgpr_count"])
        assert meta["group_segment_fixed_size"] == 0, name   # dynamic LDS only: 80 / 74 KiB are set at the launch


@pytest.mark.parametrize("kernel", sorted(PARENT_VALU))
def test_fewer_vector_instructions_than_before(kernels, kernel):
    (k,) = [v for sym, v in kernels.items() if kernel + "ItE" in sym]          # <unsigned short>: bf16 bits
    static, per_tile = PARENT_VALU[kernel]
    print(kernel, "VALU in the code", k["static"]["VALU"], "per wave and tile", k["per_tile"]["VALU"])
    assert k["static"]["VALU"] < static
    assert k["per_tile"]["VALU"] < per_tile
    assert k["per_tile"]["MFMA"] in (352, 168)           # 64 + 288 / 24 + 144: the products are all there, none twice
