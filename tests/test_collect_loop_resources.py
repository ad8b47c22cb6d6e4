"""The collection loop kernel's code object (csrc/env_collect_k0.hip, gfx950, the Makefile's flags): both
instantiations of each 16-bit format -- the default one and the profiled one -- fit four workgroups on a CU (LDS), run
one wave per SIMD, and spill no more than the kernel did before its forward and its step body became called
functions: 190 VGPRs and 644 SGPRs (profiles/default_obs_bench_pairs.txt), by the compiler's
kernel-resource-usage remarks.  The remarks cover kernels only: what the called forward and body save and spill is in
their frames, which the kernel's scratch size (printed) includes.  Compiles the unit's device code once (minutes on
one core); no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "reinforcement-learning_amd")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# Makefile: CXXFLAGS + STRICT_FP + ENV_FLAGS of env_collect_k0
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize"]
MAX_LDS, MAX_VGPR_SPILLS, MAX_SGPR_SPILLS = 40960, 190, 644


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel symbol: {remark key: value}} of the unit's device code"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("collect_loop") / "env_collect_k0.s"
    r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                        "csrc/env_collect_k0.hip", "-o", str(out)], cwd=PKG, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    fns, fn = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            fn = fns.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z\[\]/ ]+): (\d+)", line)
        if m and fn is not None:
            fn[m.group(1).strip()] = int(m.group(2))
    return fns


@pytest.mark.parametrize("split", (0, 1), ids=("default", "profiled"))
@pytest.mark.parametrize("f16", (0, 1), ids=("bf16", "fp16"))
def test_loop_kernel_resources(usage, f16, split):
    targs = "env_collect_a0ILb%dELb%dEE" % (f16, split)  # <F16, SPLIT>
    got = [d for name, d in usage.items() if targs in name]
    assert len(got) == 1, sorted(n for n in usage if "collect" in n)
    k = got[0]
    print("env_collect_a0<%d, %d>: VGPR spills %d, SGPR spills %d, scratch %d B/lane, LDS %d B, %d wave(s) per SIMD"
          % (f16, split, k["VGPRs Spill"], k["SGPRs Spill"], k["ScratchSize [bytes/lane]"], k["LDS Size [bytes/block]"],
             k["Occupancy [waves/SIMD]"]))
    assert k["LDS Size [bytes/block]"] <= MAX_LDS
    assert k["Occupancy [waves/SIMD]"] == 1
    assert k["VGPRs Spill"] <= MAX_VGPR_SPILLS
    assert k["SGPRs Spill"] <= MAX_SGPR_SPILLS
