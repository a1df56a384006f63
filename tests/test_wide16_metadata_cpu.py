"""Register and scratch budgets of the 16x16x32 wide conv tile (csrc/conv_glds_wide16.hip), on the CPU: hipcc cross-compiles gfx950 without a GPU.
The kernel lives on two workgroups of four waves per CU, i.e. 256 registers per lane, and on a K loop without a single scratch access (a spilled
LDS-DMA offset is reloaded behind a vmcnt(0), which drains the weight stream: conv_glds_wide.hip).  Read from the kernel metadata of the `-S` output only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "terrain_diffusion_amd", "csrc")


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("w16")
    (d / "u.hip").write_text('#include <hip/hip_runtime.h>\n#include <algorithm>\n#include "%s"\n' % os.path.join(CSRC, "conv_glds_wide16.hip"))
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, "--cuda-device-only", "-S", str(d / "u.hip"), "-o", str(d / "u.s")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = (d / "u.s").read_text()
    md = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - ", md)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:   # (the list of version numbers that follows the kernels has none)
            kernels[name.group(1)] ={k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, flags=re.M)}
    return kernels


def test_both_instantiations_fit_256_registers_without_scratch_or_spills(metadata):
    mine = {k: v for k, v in metadata.items() if "conv_glds_kernel_x16" in k}
    assert len(mine) == 2 and any("DF16b" in k for k in mine) and any("DF16_" in k for k in mine), sorted(metadata)   # bf16 and fp16
    assert not any(k.startswith("_ZN2td21conv_glds_kernel_wide") for k in metadata)    # the name test_isa_contract.py counts stays that file's own
    for name, f in mine.items():
        print(name, {k: f[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})
        assert f["vgpr_count"] <= 256, (name, f["vgpr_count"])
        assert f["private_segment_fixed_size"] == 0, (name, f["private_segment_fixed_size"])
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f["vgpr_spill_count"], f["sgpr_spill_count"])
        assert f["max_flat_workgroup_size"] == 256, name
