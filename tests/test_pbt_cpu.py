"""Population-based training without a GPU: the plan of one generation (avddpg_amd.pbt.plan), its ranking, the refusals of check_pbt
and of `tr --pbt`, which all come before any launch."""
import math
import re

import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import config, pbt, vec

KEYS = ["actor_lr", "gamma"]


def _rows(E):
    conf = config.Config()
    return vec.hparams_rows(conf, [dict(actor_lr=1e-4 * (1 + e), gamma=0.5 + 0.007 * e) for e in range(E)])


def _fit(E):
    return [float((7 * e) % E) for e in range(E)]  # a permutation of 0..E-1


def test_plan_is_deterministic_and_keyed_by_seeds_and_generation():
    E = 12
    args = (_fit(E), _rows(E), KEYS)
    a = pbt.plan(*args, 3, (1, 2), 0.25, (0.8, 1.2))
    assert a == pbt.plan(*args, 3, (1, 2), 0.25, (0.8, 1.2))
    draws = {repr(pbt.plan(*args, g, key, 0.25, (0.5, 0.8, 1.2, 2.0))) for g in range(1, 6) for key in ((1, 2), (3, 4))}
    assert len(draws) > 1


def test_plan_leaves_the_global_numpy_stream_alone():
    import numpy as np

    np.random.seed(5)
    want = np.random.random_sample()
    np.random.seed(5)
    pbt.plan(_fit(8), _rows(8), KEYS, 1, (9,), 0.5, (0.8, 1.2))
    assert np.random.random_sample() == want


@pytest.mark.parametrize("E,fraction", [(4, 0.25), (8, 0.25), (12, 0.5), (9, 0.3), (64, 0.25)])
def test_plan_replaces_the_bottom_k_from_the_top_k(E, fraction):
    fit, rows = _fit(E), _rows(E)
    perturb = (0.8, 1.2)
    for g in range(1, 4):
        pairs, new = pbt.plan(fit, rows, KEYS, g, (1, 2, 3), fraction, perturb)
        k = math.floor(fraction * E)
        order = pbt.ranking(fit)
        top, bottom = set(order[:k]), set(order[E - k:])
        dsts = [d for _, d in pairs]
        assert len(pairs) == k and len(set(dsts)) == k and set(dsts) == bottom
        assert all(s in top for s, _ in pairs)
        for s, d in pairs:
            for n in vec.HP_KEYS:
                if n in KEYS:
                    cand = [rows[s][n] * f for f in perturb]
                    if n in pbt.CLAMP_TO_ONE:
                        cand = [min(c, 1.0) for c in cand]
                    assert new[d][n] in cand, (n, new[d][n], cand)
                else:
                    assert new[d][n] == rows[s][n]  # not swept: inherited unchanged
        for e in range(E):
            if e not in bottom:
                assert new[e] == rows[e]
        vec.hparams_rows(config.Config(), new)  # every new row is valid


def test_plan_clamps_tau_and_gamma_to_one():
    conf = config.Config()
    rows = vec.hparams_rows(conf, [dict(tau=0.9, gamma=0.95), dict(tau=0.5, gamma=0.5)])
    pairs, new = pbt.plan([2.0, 1.0], rows, ["tau", "gamma"], 1, (1,), 0.5, (1.5,))
    assert pairs == [(0, 1)] and new[1]["tau"] == 1.0 and new[1]["gamma"] == 1.0
    vec.hparams_rows(conf, new)


def test_ranking_puts_nan_last_and_breaks_ties_by_index():
    nan = float("nan")
    assert pbt.ranking([1.0, nan, 3.0, 1.0, nan, 3.0]) == [2, 5, 0, 3, 1, 4]
    assert pbt.ranking([-5.0, -1.0, -1.0]) == [1, 2, 0]
    # a NaN experiment is replaced before any finite one
    pairs, _ = pbt.plan([nan, 0.0, 1.0, 2.0], _rows(4), KEYS, 1, (1,), 0.25, (1.0,))
    assert pairs[0][1] == 0 and pairs[0][0] == 3


@pytest.mark.parametrize("kw,msg", [
    (dict(fraction=0.0), r"\(0, 0.5\]"),
    (dict(fraction=0.6), r"\(0, 0.5\]"),
    (dict(fraction=-0.1), r"\(0, 0.5\]"),
    (dict(fraction=0.1, n_experiments=4), "replaces none"),
    (dict(perturb=(0.8, float("inf"))), "finite"),
    (dict(perturb=(0.8, float("nan"))), "finite"),
    (dict(perturb=(0.0, 1.2)), "> 0"),
    (dict(perturb=(-1.0,)), "> 0"),
    (dict(perturb=()), "empty"),
    (dict(interval=0), ">= 1"),
    (dict(interval=-5), ">= 1"),
    (dict(swept=None), "needs a hyperparameter sweep"),
    (dict(swept=[]), "needs a hyperparameter sweep"),
])
def test_check_pbt_refusals(kw, msg):
    a = dict(interval=100, fraction=0.25, perturb=(0.8, 1.2), n_experiments=8, swept=["actor_lr"])
    a.update(kw)
    with pytest.raises(ValueError, match=msg):
        pbt.check_pbt(**a)


def test_check_pbt_accepts_and_normalises():
    assert pbt.check_pbt(20000, 0.25, [0.8, 1.2], 12, ["actor_lr", "critic_lr"]) == (20000, 0.25, (0.8, 1.2), 3)


def test_cli_parses_pbt_flags():
    args, _ = cli.get_cmdl_args(["tr", "--rng", "device", "--episodes", "platoon", "--sweep", "actor_lr=5e-5,1e-4", "--sweep",
                                 "critic_lr=1e-3,2e-3", "--seeds", "1-2", "--pbt", "100", "--pbt_fraction", "0.5", "--pbt_perturb",
                                 "0.5,2"], config.Config())
    assert (args.pbt, args.pbt_fraction, args.pbt_perturb) == (100, 0.5, (0.5, 2.0))
    args, _ = cli.get_cmdl_args(["tr", "--rng", "device", "--episodes", "platoon", "--sweep", "actor_lr=5e-5,1e-4", "--seeds", "1-2",
                                 "--pbt", "100"], config.Config())
    assert (args.pbt_fraction, args.pbt_perturb) == (0.25, (0.8, 1.2))


@pytest.mark.parametrize("extra,msg", [
    (["--pbt", "100"], "needs a hyperparameter sweep"),
    (["--sweep", "tau=0.1,0.2", "--pbt", "0"], ">= 1"),
    (["--sweep", "tau=0.1,0.2", "--pbt", "10", "--pbt_fraction", "0.2"], "replaces none"),
    (["--sweep", "tau=0.1,0.2", "--pbt", "10", "--pbt_fraction", "0.75"], r"\(0, 0.5\]"),
    (["--sweep", "tau=0.1,0.2", "--pbt", "10", "--pbt_perturb", "0.8,x"], "not a comma-separated"),
    (["--sweep", "tau=0.1,0.2", "--pbt", "10", "--pbt_perturb", "0.8,-1"], "> 0"),
    (["--sweep", "tau=0.1,0.2", "--pbt_fraction", "0.5"], "need --pbt"),
])
def test_cli_refuses_pbt_before_touching_the_gpu(extra, msg, capsys, monkeypatch):
    from avddpg_amd import _hip, trainer

    monkeypatch.setattr(_hip, "call", lambda *a: pytest.fail("a C-ABI call"))
    monkeypatch.setattr(trainer, "VecTrainer", lambda *a, **k: pytest.fail("a trainer was built"))
    with pytest.raises(SystemExit):
        cli.main(["tr", "--rng", "device", "--episodes", "platoon", "--seeds", "1-2", "--out", "/nonexistent/never", *extra])
    assert re.search(msg, capsys.readouterr().err)
