"""`tr --warm_start SPEC --actor_hold N` end to end: what conf.json (and best/conf.json) record, the step-0 snapshot of --keep_best, a
seed batch against its solo runs, and a run without the flags beside one with them."""
import json
import os

import numpy as np
import pytest

from avddpg_amd import scenarios
from tests.gpu_util import need_gpu
from tests.test_gpu_residual import TR, _files, _run

pytestmark = pytest.mark.gpu

WARM = ("--warm_start", "kp=2,kv=1,steps=30", "--actor_hold", "5", "--keep_best", "40", "--fed_method", "interfrl", "--engine", "per_agent")


def _conf(d):
    return json.load(open(os.path.join(d, "conf.json")))


def test_cli_records_the_fit_and_a_seed_batch_equals_its_solo_runs(tmp_path, capsys):
    need_gpu()
    solo = {k: _run(capsys, *TR, *WARM, "--seed", str(k), "--out", str(tmp_path / f"solo{k}"))[-1] for k in (1, 2)}
    cj = _conf(solo[1])
    rec = dict(cj["warm_start"])
    assert list(rec) == ["law", "fit_loss", "evaluator_score"] and cj["actor_hold"] == 5
    law = scenarios.WarmStart.from_record(rec["law"])
    assert (law.kp, law.kv, law.steps, law.lr, law.source) == (2.0, 1.0, 30, 1e-3, "given")
    assert 0 < rec["fit_loss"] < 4.0 and np.isfinite(rec["evaluator_score"])
    # curve.csv's step-0 evaluator score is the fitted actors' (platoon 1's sets are every platoon's after the fit)
    curve = open(os.path.join(solo[1], "curve.csv")).read().splitlines()
    assert float(curve[1].split(",")[4]) == pytest.approx(rec["evaluator_score"], abs=5e-4)
    # best/: the record travels; the step-0 snapshot scored the fitted actors
    bj = _conf(os.path.join(solo[1], "best"))
    assert bj["warm_start"] == cj["warm_start"] and bj["actor_hold"] == 5
    best = open(os.path.join(solo[1], "best.csv")).read().splitlines()
    assert best[0] == "unit,best_step,best_score,final_score" and len(best) >= 2
    # a seed batch: experiment k is the solo run --seed k, file for file
    batch = _run(capsys, *TR, *WARM, "--seeds", "1,2", "--out", str(tmp_path / "batch"))[-1]
    for k in (1, 2):
        d = os.path.join(batch, f"seed{k}")
        a, b = _files(solo[k]), _files(d)
        assert set(a) == set(b) and "curve.csv" in a
        for f in a:
            assert a[f] == b[f], (k, f)
        assert _conf(d)["warm_start"] == _conf(solo[k])["warm_start"] and _conf(d)["actor_hold"] == 5
    assert _conf(solo[1])["warm_start"] != _conf(solo[2])["warm_start"]  # (each seed draws its own fit rows)
    # without the flags: no record, and another run
    plain = _run(capsys, *TR, *WARM[4:], "--seed", "1", "--out", str(tmp_path / "plain"))[-1]
    pj = _conf(plain)
    assert "warm_start" not in pj and "actor_hold" not in pj
    assert _files(plain)["curve.csv"] != _files(solo[1])["curve.csv"]
