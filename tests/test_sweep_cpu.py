"""Hyperparameter sweeps without a GPU: `tr --sweep` parsing, experiment order and labels, the avd_hparams mirror, the host-side
roundings of the table and the refusals of trainer.check_sweep."""
import ctypes
import math
import re

import numpy as np
import pytest

from avddpg_amd import __main__ as cli
from avddpg_amd import _hip, config, trainer, vec


def test_parse_sweep_and_experiment_order():
    sw = cli.parse_sweep(["actor_lr=5e-5,1e-4", "gamma=0.95,0.99,1"])
    assert sw == [("actor_lr", [5e-5, 1e-4]), ("gamma", [0.95, 0.99, 1.0])]
    exps = cli.sweep_experiments(sw, [3, 4])
    assert len(exps) == 12
    # the last flag varies fastest, the seeds innermost
    assert [(h["actor_lr"], h["gamma"], k) for _, h, k in exps[:4]] == [(5e-5, 0.95, 3), (5e-5, 0.95, 4), (5e-5, 0.99, 3), (5e-5, 0.99, 4)]
    assert exps[6][1] == {"actor_lr": 1e-4, "gamma": 0.95}
    assert exps[6][0] == "actor_lr=0.0001_gamma=0.95" and exps[0][0] == "actor_lr=5e-05_gamma=0.95"
    assert len({lab for lab, _, _ in exps}) == 6


@pytest.mark.parametrize("items,msg", [
    (["lr=1,2"], "NAME"),
    (["actor_lr"], "NAME"),
    (["actor_lr=1e-4", "actor_lr=2e-4"], "twice"),
    (["tau="], "empty"),
    (["tau=0.1,,0.2"], "empty"),
    (["tau=0.1,0.1"], "listed twice"),
    (["tau=0.1,abc"], "not a number"),
])
def test_parse_sweep_errors(items, msg):
    with pytest.raises(ValueError, match=msg):
        cli.parse_sweep(items)


def test_cli_refuses_a_sweep_without_device_platoon_flags(capsys):
    conf = config.Config()
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", "--sweep", "tau=0.1,0.2"], conf)
    assert "--rng device --episodes platoon" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", "--rng", "device", "--episodes", "platoon", "--sweep", "tau=0.1,x"], config.Config())
    with pytest.raises(SystemExit):
        cli.get_cmdl_args(["tr", "--rng", "device", "--episodes", "platoon", "--sweep", "actor_lr=1e-4,2e-4", "--actor_lr", "3e-4"],
                          config.Config())
    assert "mutually exclusive" in capsys.readouterr().err
    with pytest.raises(SystemExit):  # (an abbreviation argparse accepts)
        cli.get_cmdl_args(["tr", "--rng", "device", "--episodes", "platoon", "--sweep", "critic_lr=1e-3,2e-3", "--critic", "3e-3"],
                          config.Config())
    assert "mutually exclusive" in capsys.readouterr().err
    args, _ = cli.get_cmdl_args(["tr", "--rng", "device", "--episodes", "platoon", "--sweep", "tau=0.1,0.2", "--seeds", "1-2"],
                                config.Config())
    assert args.sweep == [("tau", [0.1, 0.2])] and args.seeds == [1, 2]


def test_hparams_struct_matches_the_header():
    assert ctypes.sizeof(_hip.HParams) == 32
    names = [n for n, _ in _hip.HParams._fields_]
    assert names == ["actor_lr", "critic_lr", "tau", "one_minus_tau", "gamma", "ou_theta", "ou_scale", "reserved"]
    assert [getattr(_hip.HParams, n).offset for n in names] == list(range(0, 32, 4))
    text = open(_hip.HEADER_PATH).read()
    body = re.search(r"typedef struct avd_hparams \{(.*?)\} avd_hparams;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in re.findall(r"float\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert declared == names


def test_host_table_rounds_as_the_scalar_entry_points():
    conf = config.Config()
    rows = vec.hparams_rows(conf, [{"tau": 0.003, "std_dev": 0.07, "gamma": 0.95}, {}])
    tbl = np.frombuffer(bytes((_hip.HParams * 2)(*[vec.hparams_struct(r, conf.ou_dt) for r in rows])), dtype=np.float32).reshape(2, 8)
    f32 = np.float32
    for row, got in zip(rows, tbl):
        want = [f32(row["actor_lr"]), f32(row["critic_lr"]), f32(row["tau"]), f32(1.0 - row["tau"]), f32(row["gamma"]),
                f32(row["theta"]), f32(row["std_dev"]) * f32(math.sqrt(float(f32(conf.ou_dt)))), f32(0)]
        assert got.view(np.int32).tolist() == np.array(want, dtype=np.float32).view(np.int32).tolist()
    assert rows[1] == {k: float(getattr(conf, k)) for k in vec.HP_KEYS}


@pytest.mark.parametrize("hp,kw,msg", [
    ([{"lr": 1.0}], {}, "unknown key"),
    ([{"gamma": float("nan")}], {}, "not finite"),
    ([{"actor_lr": 0.0}], {}, "> 0"),
    ([{"critic_lr": -1e-3}], {}, "> 0"),
    ([{"tau": 0.0}], {}, r"\(0, 1\]"),
    ([{"tau": 1.5}], {}, r"\(0, 1\]"),
    ([{"gamma": 1.01}], {}, r"\[0, 1\]"),
    ([{"std_dev": -0.1}], {}, ">= 0"),
    ([{"theta": -0.1}], {}, ">= 0"),
    ([{}], dict(shared_engine="fused"), "per_agent"),
    ([{}], dict(shared_engine="batched"), "per_agent"),
    ([{}], dict(pipeline_chunks=4), "pipeline"),
    ([{}, {}], {}, "rows for"),
])
def test_check_sweep_refusals(hp, kw, msg):
    with pytest.raises(ValueError, match=msg):
        trainer.check_sweep(config.Config(), (1,), hp, **kw)


def test_check_sweep_widths_and_repeats():
    with pytest.raises(ValueError, match="reference widths"):
        trainer.check_sweep(config.Config(actor_layer1_size=128, critic_layer1_size=128), (1,), [{}])
    with pytest.raises(ValueError, match="twice"):
        trainer.check_sweep(config.Config(), (1, 1), [{"tau": 0.1}, {"tau": 0.1}])
    rows = trainer.check_sweep(config.Config(), (1, 1), [{"tau": 0.1}, {"tau": 0.2}])  # a seed may repeat with other values
    assert [r["tau"] for r in rows] == [0.1, 0.2]
    with pytest.raises(ValueError, match="duplicate"):  # a plain seed batch still refuses repeats
        vec.seed_table((1, 1), "cpu")
    assert vec.seed_table((1, 1), "cpu", distinct=False)[0] == (1, 1)
