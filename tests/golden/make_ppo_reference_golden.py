"""Generates tests/golden/ppo_reference.npz: the float64 PPO minibatch reference of every case of the training-kernel
tests, as ppo_reference.golden_record keeps it (six metrics, six scales, head_bias_scale, guiding and guide_scale where
present, per parameter tensor ||g|| and g . u) -- scalars only, no gradients.

The committed file was produced by this script from the three separate statements of the reference (test_ppo_variants'
minibatch_ref, test_policy_options' minibatch_ref_opt, test_guiding_policy's minibatch_ref_guide) in the commit before
ppo_reference.minibatch_ref replaced them, through the same case_data / option_data / guide_data / act_case calls as
below; test_reference_matches_golden holds the one function to it.  Re-run only when a case table changes on
purpose: python tests/golden/make_ppo_reference_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (TESTS, ROOT, os.path.join(ROOT, "reinforcement-learning_amd")):
    sys.path.insert(0, p)
import ppo_reference  # noqa: E402
import test_activations as A  # noqa: E402
import test_guiding_policy as G  # noqa: E402
import test_policy_options as O  # noqa: E402
import test_ppo_variants as V  # noqa: E402


def cases():
    """(key, case data) of every pinned case; the keys are test_reference_matches_golden's."""
    for name in V.CASES:
        yield f"plain/{name}", V.case_data(name)
    for name in O.OPTION_CASES:
        yield f"option/{name}", O.option_data(name)
    for name in list(G.GUIDE_CASES) + ["rows8161"]:
        yield f"guide/{name}", G.guide_data(name)
    for name in A.GOLDEN_CASES:
        for act in A.ACTS:
            yield f"act/{name}/{act}", A.act_case(name, act)


def main():
    out, n = {}, 0
    for key, d in cases():
        for field, value in ppo_reference.golden_record(d["r64"], d["mods"]).items():
            out[f"{key}:{field}"] = value
        n += 1
    np.savez_compressed(ppo_reference.GOLDEN, **out)
    print("wrote", n, "cases,", os.path.getsize(ppo_reference.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
