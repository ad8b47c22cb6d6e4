"""The full-row H3 input-gradient GEMM with the LayerNorm + LeakyReLU backward of the layer below in the same
launch (mlp::gemm_h3_row_lnbwd, RLGPU_H3_ROWFUSE_BWD) against the two-kernel path it replaces (gemm_x6 +
ln_act_bwd<8>): same bits, the launches it is meant to replace and no others, and a kernel that keeps its
registers and its two workgroups per CU."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "reinforcement-learning_amd")

BASE = dict(num_actions=90, policy_layers=(512, 512), critic_layers=(512, 512), layer_norm=True, leaky_slope=0.01,
            shared_layers=())


def _case(rows, ln_bwd, **kw):
    """rows: the minibatches of one model, run without zero_grad in between.  ln_bwd: stand-alone LayerNorm
    backward launches per minibatch with the knob at (0, 1)."""
    return dict(BASE, rows=rows if isinstance(rows, tuple) else (rows,), ln_bwd=ln_bwd, **kw)


# The kernel's tile is 64 rows, its dA stage and partial block 32 rows.  The default model has 4 LayerNorm
# backward launches per minibatch; fused, only the critic's last one (rank-1 head variant, no GEMM in front)
# is left.
CASES = [_case(n, (4, 1)) for n in (1, 31, 33, 63, 65, 97)]  # half and tile edges
CASES += [
    _case(1000, (4, 1)),                  # 15 whole blocks and a ragged one of 40 rows
    _case(97, (4, 1), num_actions=20),    # head dA: K = 20, one short stage
    _case(97, (4, 1), num_actions=128),   # K = 128, a multiple of 32 (K = 90, rows of 92 floats: the default)
    _case(97, (5, 1), policy_layers=(512, 512, 512)),  # two chained K = 512 launches behind the head's: the ping-pong
    # the dA of a 510-input layer is not eligible: the head's launch is fused, the first layers keep their own
    _case(97, (4, 3), policy_layers=(510, 512), critic_layers=(510, 512)),
    # 510-column dZ rows (ragged leading dimension) and a 510-wide consumer: everything falls back
    _case(97, (4, 4), policy_layers=(512, 510), critic_layers=(512, 510)),
    _case(65, (4, 1), layer_norm=False),
    _case(193, (4, 1), leaky_slope=0.2),
    # behind a shared head the first layers' dA is the model-input gradient (dX -> dshared): no LayerNorm follows
    # it in that model, so only the policy head's launch is fused
    _case(97, (3, 2), shared_layers=(512,), policy_layers=(512,), critic_layers=(512,)),
    _case((1000, 65), (4, 1)),            # stale rows / buffers of an earlier, larger call
]

_CHILD = r"""
import json, sys, numpy as np, torch
sys.path[:0] = [sys.argv[2], sys.argv[2] + "/reinforcement-learning_amd", sys.argv[2] + "/tests"]
from rlgpu.ppo import PPO, kernel_timing, kernel_timing_read
from test_ppo import make_batch
from test_ppo_rowfuse_bwd import CASES
dev = torch.device("cuda:0")
out, counts = [], []
for k, c in enumerate(CASES):
    p = PPO(num_actions=c["num_actions"], policy_layers=c["policy_layers"], critic_layers=c["critic_layers"],
            layer_norm=c["layer_norm"], leaky_slope=c["leaky_slope"], shared_layers=c["shared_layers"], max_rows=1024, seed=5)
    p.zero_grad()
    kernel_timing(True)
    for i, n in enumerate(c["rows"]):
        obs, masks, acts, old, adv, tgt = make_batch(np.random.default_rng(1000 * k + n), n, A=c["num_actions"])
        d = [torch.from_numpy(v).to(dev) for v in (obs, masks, acts, old, adv, tgt)]
        if n > 1 and i == 0:
            p.adv_normalizer(d[4])
        p.minibatch(*d, None, 0, n, n)
    torch.cuda.synchronize()
    counts.append(kernel_timing_read()["LayerNorm backward"][2])
    kernel_timing(False)
    out.append(p.flat(grads=True).cpu().numpy())
np.save(sys.argv[1], np.concatenate(out))
json.dump(counts, open(sys.argv[1] + ".json", "w"))
"""


@pytest.mark.gpu
@pytest.mark.timeout(240)
def test_rowfuse_bwd_bit_identical(gpu, tmp_path):
    """RLGPU_H3_ROWFUSE_BWD=1 (every eligible dA GEMM + LayerNorm backward pair on gemm_h3_row_lnbwd) gives the
    same minibatch gradients, bit for bit, as RLGPU_H3_ROWFUSE_BWD=0 (gemm_x6 + ln_act_bwd): the same products
    in the same order into one accumulator, the same epilogue value, the LayerNorm backward's own row arithmetic
    on those bits, and its row-to-wave assignment and partial blocks.  The stand-alone LayerNorm backward
    launches that remain (the learn-phase timing spans count them) show that the fused launch ran where it
    should and nowhere else.  The knob is read once per process: child processes."""
    res, cnt = {}, {}
    for v in ("0", "1"):
        f = str(tmp_path / f"r{v}.npy")
        r = subprocess.run(["timeout", "-k", "10", "90", sys.executable, "-c", _CHILD, f, ROOT],
                           env=dict(os.environ, RLGPU_H3_ROWFUSE_BWD=v), capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res[v] = np.load(f)
        cnt[v] = json.load(open(f + ".json"))
    for v, col in (("0", 0), ("1", 1)):
        assert cnt[v] == [c["ln_bwd"][col] * len(c["rows"]) for c in CASES], (v, cnt[v])
    assert res["0"].shape == res["1"].shape
    assert np.isfinite(res["0"]).all() and np.isfinite(res["1"]).all()
    np.testing.assert_array_equal(res["0"].view(np.uint32), res["1"].view(np.uint32))


def test_rowfuse_bwd_kernel_resources(tmp_path):
    """The compiler's resource-usage remarks for gemm_h3_row_lnbwd (device code of csrc/mlp_kernels.hpp alone, the
    library's flags): no spill, no scratch, and two workgroups per CU -- 256 threads with at most 256 registers
    (2 waves / SIMD) and at most half of the CU's 160 KB of LDS."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    src = tmp_path / "rowlnb.hip"
    src.write_text('#include "%s"\n' % os.path.join(PKG, "csrc", "mlp_kernels.hpp"))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", str(src), "-o", str(tmp_path / "rowlnb.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = r.stderr.split("Function Name: ")
    mine = [b for b in blocks if "gemm_h3_row_lnbwd" in b.splitlines()[0]]
    assert len(mine) == 1, [b.splitlines()[0] for b in blocks[1:]]
    val = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", mine[0])}
    print(val)
    assert val["VGPRs Spill"] == 0 and val["SGPRs Spill"] == 0 and val["ScratchSize"] == 0, val
    assert val["VGPRs"] + val["AGPRs"] <= 256 and val["Occupancy"] >= 2, val
    assert val["LDS Size"] <= 80 * 1024, val
