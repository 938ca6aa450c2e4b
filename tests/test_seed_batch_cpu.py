"""Seed batches without a device: `--seeds` parsing and usage errors, the interleaved lane mapping, the guard rails."""
import itertools

import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import config, trainer, vec


def test_parse_seeds_lists_and_ranges():
    assert cli.parse_seeds("1,2,5-8") == [1, 2, 5, 6, 7, 8]
    assert cli.parse_seeds("7") == [7]
    assert cli.parse_seeds("3-3,0") == [3, 0]
    assert cli.parse_seeds(" 4 , 2-3 ") == [4, 2, 3]
    assert cli.parse_seeds(f"{2 ** 32 - 1}") == [2 ** 32 - 1]


@pytest.mark.parametrize("bad", ["", "1,,2", "a", "1-", "-3", "5-2", "1,2,1", "1-4,3", "2.5", f"{2 ** 32}"])
def test_parse_seeds_rejects(bad):
    with pytest.raises(ValueError):
        cli.parse_seeds(bad)


@pytest.mark.parametrize("argv", [
    ["tr", "--seeds", "1,2"],                                                # host RNG, reference episodes
    ["tr", "--seeds", "1,2", "--rng", "device"],                             # reference episodes
    ["tr", "--seeds", "1,2", "--episodes", "platoon"],                       # host RNG
    ["tr", "--seeds", "1,1", "--rng", "device", "--episodes", "platoon"],    # duplicate
    ["tr", "--seeds", "2-1", "--rng", "device", "--episodes", "platoon"],    # reversed range
    ["tr", "--seeds", "1,2", "--seed", "3", "--rng", "device", "--episodes", "platoon"],
])
def test_seeds_usage_errors(argv):
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(argv, config.Config())


def test_seeds_argument_parsed():
    args, _ = cli.get_cmdl_args(["tr", "--seeds", "1,5-6", "--rng", "device", "--episodes", "platoon"], config.Config())
    assert args.seeds == [1, 5, 6]
    args, _ = cli.get_cmdl_args(["tr", "--seed", "4"], config.Config())
    assert args.seeds is None and args.seed == 4


def test_lane_mapping_against_enumeration():
    """Agent (e, p, m) of a batch of E experiments is v = (p*E + e)*M + m; its draws use the solo run's indices: platoon p, vehicle
    p*L + i, agent p*M + m, replay thread (p*M + m)*(B/4) + q. The kernels' formulas (csrc/env.hip seed_key, csrc/replay.hip) are
    restated and checked against the enumeration."""
    for E, P, M, B in itertools.product((1, 2, 3, 5), (1, 4, 7), (1, 3, 5), (4, 64)):
        seen = set()
        for e, p, m in itertools.product(range(E), range(P), range(M)):
            g = vec.batch_platoon(e, p, E)
            v = g * M + m
            assert vec.lane_of(g, E) == (e, p)
            assert g // E == p and g % E == e and v // M == g
            for q in range(B // 4):
                base = v * B + 4 * q  # the batch thread t = base / 4 of replay_sample_kernel
                ag = base // B
                gg = ag // M
                ti = ((gg // E) * M + (ag - gg * M)) * (B // 4) + (base - ag * B) // 4
                assert (gg % E, ti) == (e, (p * M + m) * (B // 4) + q)
            seen.add(v)
        assert seen == set(range(E * P * M))


def test_seed_table():
    seeds, d = vec.seed_table([5, 17, 2 ** 40 + 3, 2 ** 64 - 1], "cpu")
    assert seeds == (5, 17, 2 ** 40 + 3, 2 ** 64 - 1)
    assert [int(x) & (2 ** 64 - 1) for x in d.tolist()] == list(seeds)
    for bad in ([], [1, 1], [-1], [2 ** 64]):
        with pytest.raises(ValueError):
            vec.seed_table(bad, "cpu")


@pytest.mark.parametrize("ckw,tkw,msg", [
    (dict(), dict(rng="host"), "rng='device'"),
    (dict(), dict(auto_reset=True), "per-platoon episodes"),
    (dict(), dict(auto_reset=False), "per-platoon episodes"),
    (dict(framework="centralized", pl_size=1), dict(), "decentralized"),
    (dict(fed_method="intrafrl"), dict(), "intrafrl"),
    (dict(fed_method="interfrl", aggregation_method="weights"), dict(), "gradient aggregation"),
    (dict(), dict(group=object()), "process group"),
    (dict(), dict(fused_step=False), "fused step"),
    (dict(), dict(seed=3), "mutually exclusive"),
    (dict(), dict(init_seed=3), "mutually exclusive"),
    (dict(), dict(seeds=(1, 1)), "duplicate"),
])
def test_rejected_batches_raise_before_touching_the_device(ckw, tkw, msg):
    """Every combination a batch cannot run raises in VecTrainer's first lines -- no allocation, no launch (no device needed)."""
    conf = config.Config(num_platoons=2, **{"pl_size": 3, **ckw})
    kw = dict(rng="device", auto_reset="platoon", seeds=(1, 2), device="cpu")
    kw.update(tkw)
    with pytest.raises(ValueError, match=msg):
        trainer.VecTrainer(conf, **kw)
