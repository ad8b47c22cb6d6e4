"""The rollout collection's arena groups on disjoint CU partitions (host/cu_partition.cpp, Learner::CollectGrouped).

  * Partition: streams made for G = 2, 4, 8 groups place whole-SIMD workgroups (rlgpu_debug_cu_probe: one wave
    holding all 512 registers per lane, as an env workgroup does) on pairwise disjoint CU sets, the same number of
    CUs in every XCD for every group, inside the device, and inside the mask the runtime reports for the stream.
    How mask bits map to physical CUs is not documented, so "inside the mask" is checked by what is observable:
    the reported mask is the partition's own, the stream reaches exactly as many CUs as its mask has bits, and
    -- the masks being nested, mask(G, g) = mask(2G, g) | mask(2G, g + G) -- a CU seen in group g of 2G groups is
    seen in group g % G of G groups.
  * Bit identity: at 64 arenas (the smallest count divisible by 4 G for G = 8: two env workgroups per group), T = 8,
    default models, two iterations with collect_groups = 2, 4, 8 and 0 (automatic) leave every rollout array and
    the flat parameters byte-equal to collect_groups = 1; once with an old version playing one team; with a step
    hook the collection reports one group; an arena count not divisible by 4 G reports one group too.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GROUPS = (2, 4, 8)
ARRAYS = ("obs", "masks", "actions", "logp", "rewards", "terms", "trunc_obs", "values", "trunc_vals", "adv", "target",
          "ret")


# ------------------------------------------------------------------ partition
@pytest.fixture(scope="module")
def placement(gpu):
    """{0: CUs of an unmasked launch, G: [per group: (requested mask, reported mask, set of (xcd, se, cu))]}."""
    import torch
    from rlgpu import partition
    ncu = torch.cuda.get_device_properties(gpu).multi_processor_count

    def cus(rows):
        assert (rows[:, 0] != 0xFFFFFFFF).all(), "a probe workgroup did not report"
        return {tuple(int(x) for x in r[:3]) for r in rows}

    seen = {0: cus(partition.probe(None, 4 * ncu, hold_us=500)), "ncu": ncu}
    for G in GROUPS:
        want = partition.masks(ncu, G)
        seen[G] = []
        for g in range(G):
            s = partition.PartitionStream(G, g)
            try:
                seen[G].append((want[g], s.mask(), cus(partition.probe(s.stream, 4 * ncu // G, hold_us=500))))
            finally:
                s.close()
    return seen


def test_unmasked_launch_reaches_every_cu(placement):
    assert len(placement[0]) == placement["ncu"]
    assert sorted({c[0] for c in placement[0]}) == list(range(8))


@pytest.mark.parametrize("G", GROUPS)
def test_partition_streams_are_disjoint_and_balanced(placement, G):
    from rlgpu.partition import mask_bits
    ncu, groups = placement["ncu"], placement[G]
    union = set()
    for g, (want, got, cus) in enumerate(groups):
        print(f"G={G} g={g}: {len(cus)} CUs, per XCD {[sum(c[0] == x for c in cus) for x in range(8)]}, "
              f"engines {sorted({c[1] for c in cus})}")
        np.testing.assert_array_equal(got, want, err_msg=f"reported mask of group {g}")
        assert len(mask_bits(got)) == ncu // G
        assert len(cus) == len(mask_bits(got)), (g, len(cus))  # as many CUs as the mask has bits
        assert not (union & cus), f"group {g} shares CUs with an earlier group"
        union |= cus
        per_xcd = [sum(c[0] == x for c in cus) for x in range(8)]
        assert per_xcd == [ncu // 8 // G] * 8, (g, per_xcd)
    assert union <= placement[0] and len(union) <= ncu


def test_partition_masks_nest_on_the_device(placement):
    """mask(G, g) = mask(2G, g) | mask(2G, g + G) bit for bit, so the CUs seen must nest the same way."""
    for G in (2, 4):
        for g in range(G):
            lo, hi = placement[2 * G][g], placement[2 * G][g + G]
            np.testing.assert_array_equal(placement[G][g][0], lo[0] | hi[0])
            assert placement[G][g][2] == lo[2] | hi[2], (G, g)


# ------------------------------------------------------------------ bit identity
def _learner(gpu, **kw):
    from rlgpu.learner import Learner, LearnerConfig
    cfg = LearnerConfig(**{**dict(num_arenas=64, rollout_len=8, mini_batch_size=512, seed=5, max_episode_duration=1.2,
                                  train_against_old_versions=False), **kw})
    return Learner(cfg, device=gpu)


def _run(L, iterations=2):
    """Per iteration: (arenas per env launch, old version, {array: bytes}, flat parameters)."""
    import torch
    out = []
    for _ in range(iterations):
        rep = L.iterate()
        torch.cuda.synchronize()
        arrays = {n: getattr(L, n).contiguous().view(torch.uint8).cpu().clone() for n in ARRAYS}
        out.append((rep["env_launch_arenas"], rep["old_version"], arrays, L.ppo.flat().view(torch.uint8).cpu().clone()))
    L.close()
    return out


_plain = {}


def _reference(gpu, **kw):
    """The one-group run of a configuration, computed once and shared."""
    key = tuple(sorted(kw.items()))
    if key not in _plain:
        _plain[key] = _run(_learner(gpu, collect_groups=1, **kw))
    return _plain[key]


def _assert_same(got, want, arenas_per_launch):
    import torch
    for it, ((la, old, arrays, flat), (_, wold, warrays, wflat)) in enumerate(zip(got, want)):
        assert la == arenas_per_launch, (it, la)
        assert old == wold, it
        for n in ARRAYS:
            assert torch.equal(arrays[n], warrays[n]), (it, n)
        assert torch.equal(flat, wflat), it


@pytest.mark.parametrize("G", (2, 4, 8))
def test_partitioned_collection_is_bit_identical(gpu, G):
    _assert_same(_run(_learner(gpu, collect_groups=G)), _reference(gpu), 64 // G)


def test_automatic_collection_is_bit_identical(gpu):
    """collect_groups = 0: whatever the automatic choice is at this size, the results are the one-group run's."""
    got = _run(_learner(gpu, collect_groups=0))
    assert got[0][0] in (64, 32, 16, 8, 4)
    _assert_same(got, _reference(gpu), got[0][0])


def test_partitioned_collection_with_an_old_version(gpu):
    """train_against_old_versions: the second iteration plays one team with an old version (the old-rows path of
    the per-group inference)."""
    kw = dict(train_against_old_versions=True, train_against_old_chance=1.0)
    want = _reference(gpu, **kw)
    assert want[0][1] is None and want[1][1] is not None
    _assert_same(_run(_learner(gpu, collect_groups=8, **kw)), want, 8)


def test_step_hook_collects_in_one_group(gpu):
    L = _learner(gpu, collect_groups=4)
    calls = []
    L.set_step_hook(calls.append)
    got = _run(L)
    assert calls == [0, 1] * 16
    _assert_same(got, _reference(gpu), 64)


def test_indivisible_arena_count_collects_in_one_group(gpu):
    """24 arenas are not a multiple of 4 G = 16: one group, the plain path."""
    _assert_same(_run(_learner(gpu, num_arenas=24, collect_groups=4)), _reference(gpu, num_arenas=24), 24)
