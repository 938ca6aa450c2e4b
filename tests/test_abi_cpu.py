"""CPU checks of the C-ABI boundary: the library loads, exports every symbol the header declares,
and the host-side structs/layout agree with it. No compute calls (no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from avddpg_amd import _hip, config, dynamics, params


def _declared():
    text = open(_hip.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", text)))


def test_library_loads_and_exports_every_declared_symbol():
    lib = _hip.lib()
    names = _declared()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/avddpg_hip.h but not exported"
    assert lib.avd_version() >= 1
    # every int-returning entry point has a ctypes prototype in the binding
    assert set(names) - {"avd_last_error", "avd_version", "avd_diagnostics_enabled"} == set(_hip._PROTOS)


def test_dynamic_symbol_table_is_exactly_the_declared_c_abi():
    """built with -fvisibility=hidden + a linker version script, the library's dynamic symbol table holds the
    `avd_*` entry points of include/avddpg_hip.h and nothing else -- no mangled C++ helper, launcher or kernel handle."""
    import subprocess

    for path in (_hip.LIB_PATH, _hip.DIAG_LIB_PATH):
        if not os.path.exists(path):
            continue
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        syms = sorted(line.split()[-1] for line in nm.stdout.splitlines() if line.strip())
        assert syms and all(s.startswith("avd_") for s in syms), [s for s in syms if not s.startswith("avd_")]
        extra = set(syms) - set(_declared())
        assert all(s.startswith("avd_debug_") for s in extra), extra  # (phase-timing read-outs of diagnostic builds only)
        if path == _hip.LIB_PATH:
            assert set(syms) == set(_declared())
    # the f16x3 name is the real one; r03's bf16x3 stays as an alias with the same prototype
    assert _hip._PROTOS["avd_learn_set_split_bf16x3"] == _hip._PROTOS["avd_learn_set_split_f16x3"]


def test_shipped_library_reads_no_environment_switch():
    """every diagnostic switch (kernel / tile choices, work-skipping ablations) is compiled in only under
    -DAVD_DIAG (`make diag` -> libavddpg_hip_diag.so). The product library holds no "AVD_" string at all, does not import
    getenv, and says so through the C ABI; the diagnostic build holds the switches and says THAT."""
    import subprocess

    data = open(_hip.LIB_PATH, "rb").read()
    assert b"AVD_" not in data, sorted(set(re.findall(rb"AVD_[A-Z0-9_]+", data)))
    assert _hip.lib().avd_diagnostics_enabled() == 0
    nm = subprocess.run(["nm", "-D", "--undefined-only", _hip.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        assert not re.search(r"\bgetenv\b", nm.stdout), "the shipped library imports getenv"
    if os.path.exists(_hip.DIAG_LIB_PATH):
        diag = open(_hip.DIAG_LIB_PATH, "rb").read()
        assert b"AVD_FSPLIT_J" in diag and b"AVD_LEARN_KERNEL" in diag
        with _hip.diag_library() as d:
            assert d.avd_diagnostics_enabled() == 1
        assert _hip.lib().avd_diagnostics_enabled() == 0  # (the context manager restored the product library)


def test_error_reporting_without_gpu():
    with pytest.raises(_hip.AvdError, match="non-positive"):
        _hip.make_layout(4, 1, 0, 128, 48, 64)
    # argument validation happens before any HIP call
    with pytest.raises(_hip.AvdError, match="L must be"):
        _hip.call("avd_env_step_f32", None, 4, 99, None, None, None, None, None, None, None, None, None, None, None, None)
    lay = _hip.make_layout(12, 3, 307, 153, 57, 64)  # unpadded centralized widths: refused, with the remedy named
    with pytest.raises(_hip.AvdError, match="pad the widths"):
        _hip.call("avd_learn_f32", ctypes.byref(lay), 1, 0, *([None] * 8), 0.99, 2.5, None, None, None)


def test_intra_update_refuses_an_oversized_grid_before_any_launch():
    """avd_adam_polyak_intra_f32 puts P * M on grid.y of its second launch (the statistics' soft update): more than 65535 agents are
    refused with the other argument checks, ahead of the first launch, so a refused call has stepped nothing. (P <= 65535 and M <= 16
    alone let 4096 x 16 through to that second launch, after theta, m, v and theta_t had stepped.)"""
    lay = _hip.make_layout(4, 1, 256, 128, 48, 64)
    intra = lambda P, M: _hip.call("avd_adam_polyak_intra_f32", ctypes.byref(lay), P, M, 0, *([None] * 9), 1e-4, 1e-3, 0.005, None)
    with pytest.raises(_hip.AvdError, match=r"avd_adam_polyak_intra_f32: P=4096 x M=16 agents exceed the grid limit"):
        intra(4096, 16)
    with pytest.raises(_hip.AvdError, match="avd_adam_polyak_intra_f32: null pointer"):  # 65520 agents: past that check, still no launch
        intra(4095, 16)


def test_learn_shape_check_draws_the_lds_boundary_without_a_launch():
    """avd_learn_check_shape: what avd_learn_f32 / avd_learn_update_f32 would say about a shape, on the host. At 320/160/64 the general
    kernel's tile takes 36968 + 64 S + 448 A floats of the 40960: centralized pl_size 5 fits with 472 to spare, pl_size 6 does not."""
    ok = [(4, 1, 256, 128, 48), (3, 1, 256, 128, 48), (20, 5, 320, 160, 64), (64, 16, 128, 64, 32), (21, 3, 128, 256, 32), (1, 1, 16, 32, 16)]
    for dims in ok:
        lay = _hip.make_layout(*dims, 64)
        _hip.call("avd_learn_check_shape", ctypes.byref(lay))
    for dims, B, msg in (((24, 6, 320, 160, 64), 64, r"need 164768 B of LDS per 64-row tile \(> 160 KiB\)"),
                         ((4, 1, 256, 288, 48), 64, "H2 a multiple of 32 and <= 256"), ((65, 1, 256, 128, 48), 64, "S <= 64"),
                         ((4, 17, 256, 128, 48), 64, "A <= 16"), ((4, 1, 256, 128, 48), 32, "B == 64")):
        lay = _hip.make_layout(*dims, B)
        with pytest.raises(_hip.AvdError, match=msg):
            _hip.call("avd_learn_check_shape", ctypes.byref(lay))


def test_layout_matches_reference_parameter_counts():
    lay = _hip.make_layout(4, 1, 256, 128, 48, 64)
    # SURVEY a-9/a-10: 35 073 actor + 41 409 critic trainables, 768 + 864 moving stats
    d = params.logical_dims(lay)
    a = sum(int(np.prod(shp(d))) for _, k, shp in params.ACTOR_WEIGHTS if k == "t")
    c = sum(int(np.prod(shp(d))) for _, k, shp in params.CRITIC_WEIGHTS if k == "t")
    assert (a, c) == (35073, 41409)
    assert lay.actor_size == 35076 and lay.theta_size == 35076 + 41412 and lay.stats_size == 1632
    assert len(params.ACTOR_WEIGHTS) == 14 and len(params.CRITIC_WEIGHTS) == 20
    for f in _hip._LAYOUT_FIELDS[6:]:
        assert getattr(lay, f) % 4 == 0


def test_pack_unpack_roundtrip_and_init_bounds():
    lay = _hip.make_layout(3, 1, 64, 32, 16, 64)
    th, st = params.init_weights(lay, np.random.RandomState(0))
    aw = params.unpack(lay, th, st, "actor")
    cw = params.unpack(lay, th, st, "critic")
    assert [w.shape for w in aw][:2] == [(3, 64), (64,)] and cw[12].shape == (64 + 16, 32)
    assert np.abs(aw[0]).max() <= 1 / np.sqrt(64) and np.abs(aw[6]).max() <= 1 / np.sqrt(32)
    assert np.abs(aw[12]).max() <= 0.003 and np.abs(cw[18]).max() <= 0.0003
    assert np.abs(cw[2]).max() <= 1 / np.sqrt(32)  # action layer uses layer2_init (agent/model.py:70)
    assert np.all(aw[2] == 1) and np.all(aw[5] == 1) and np.all(aw[4] == 0) and np.all(aw[1] == 0)
    th2, st2 = np.zeros_like(th), np.zeros_like(st)
    params.pack(lay, aw, th2, st2, "actor")
    params.pack(lay, cw, th2, st2, "critic")
    assert np.array_equal(th, th2) and np.array_equal(st, st2)
    with pytest.raises(ValueError):
        params.pack(lay, aw[:-1], th2, st2, "actor")


def test_env_consts_match_oracle_matrices():
    from oracle import platoon

    for method in ("euler", "exact"):
        conf = config.Config(method=method, dyn_coeff=0.25, pl_leader_tau=0.15, timegap=0.8, sample_rate=0.05)
        c = dynamics.env_consts(conf, 5)
        ep = platoon.EnvParams(method=method, dyn_coeff=0.25, pl_leader_tau=0.15, timegap=0.8, sample_rate=0.05)
        A, B, Cm = platoon.platoon_matrices(ep, 5)
        for i in range(5):
            assert np.array_equal(np.array(list(c.A[i]), dtype=np.float32), A[i].astype(np.float32).ravel())
            assert np.array_equal(np.array(list(c.B[i]), dtype=np.float32), B[i].astype(np.float32))
            assert np.array_equal(np.array(list(c.C[i]), dtype=np.float32), Cm[i].astype(np.float32))
    assert ctypes.sizeof(_hip.EnvConsts) == 4 * 4 + 20 * 4 + 16 * 24 * 4
    with pytest.raises(ValueError):
        dynamics.env_consts(config.Config(), 17)


def test_config_defaults_and_derived_counts():
    c = config.Config()
    assert (c.steps_per_episode, c.number_of_episodes, c.fed_update_delay_steps) == (600, 1666, 1)
    assert c.fed_enabled is False and config.Config(fed_method="interfrl").fed_enabled is True
    with pytest.raises(AttributeError):
        config.Config(not_a_field=1)


def test_product_package_never_imports_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dirpath, _, files in os.walk(os.path.join(root, "avddpg_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "/root/reference" not in src, f


def test_philox_known_answers():
    """Random123 Philox4x32-10 known-answer vectors for the oracle's restatement of the device RNG."""
    from oracle import philox
    z = np.array([0])
    assert [int(v[0]) for v in philox.philox4x32_10(z, z, z, z, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    o = np.array([0xffffffff])
    assert [int(v[0]) for v in philox.philox4x32_10(o, o, o, o, 0xffffffff, 0xffffffff)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    idx = philox.replay_indices(3, 64, 1000, seed=1, counter=0)
    assert idx.shape == (3, 64) and idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < 1000


def test_padded_pack_unpack_roundtrip():
    """Centralized widths (int(256*1.2), int(128*1.2), int(48*1.2) = 307/153/57) live in slabs padded to 320/160/64:
    pack -> unpack is the identity on the logical tensors and the padding holds its neutral values."""
    dims = params.Dims(12, 3, 307, 153, 57)
    H1p, H2p, Hap = params.padded_widths(dims.H1, dims.H2, dims.Ha)
    assert (H1p, H2p, Hap) == (320, 160, 64)
    lay = _hip.make_layout(12, 3, H1p, H2p, Hap, 64)
    th, st = params.init_weights(lay, np.random.RandomState(0), nominal=(256, 128), dims=dims)
    for which, n_all, n_tr in (("actor", 14, 10), ("critic", 20, 14)):
        w = params.unpack(lay, th, st, which, dims=dims)
        assert len(w) == n_all
        th2, st2 = np.full_like(th, 7.0), np.full_like(st, 7.0)
        params.pack(lay, w, th2, st2, which, dims=dims)
        w2 = params.unpack(lay, th2, st2, which, dims=dims)
        for x, y in zip(w, w2):
            assert x.shape == y.shape and np.array_equal(x, y)
        assert len(params.unpack(lay, th, st, which, trainable_only=True, dims=dims)) == n_tr
    cw = params.unpack(lay, th, st, "critic", dims=dims)
    assert cw[12].shape == (307 + 57, 153) and cw[0].shape == (12, 307) and cw[18].shape == (153, 3)
    # padded columns of W1 are zero, padded gamma/var are one
    aW1 = th[lay.aW1:lay.aW1 + 12 * 320].reshape(12, 320)
    assert np.all(aW1[:, 307:] == 0) and np.all(aW1[:, :307] != 0)
    assert np.all(th[lay.ag1 + 307:lay.ag1 + 320] == 1) and np.all(st[lay.amv1 + 307:lay.amv1 + 320] == 1)
    cW2 = th[lay.actor_size + lay.cW2:lay.actor_size + lay.cW2 + 384 * 160].reshape(384, 160)
    assert np.all(cW2[307:320] == 0) and np.all(cW2[320 + 57:] == 0) and np.all(cW2[:, 153:] == 0)
    assert np.array_equal(cW2[320:377, :153], cw[12][307:])


def test_shared_learner_argument_validation_without_gpu():
    """check_wide runs before any HIP call: unsupported widths and bad agent counts are refused with the rule named."""
    need = ctypes.c_size_t(0)
    lay = _hip.make_layout(4, 1, 320, 160, 48, 64)
    with pytest.raises(_hip.AvdError, match="multiples of 64"):
        _hip.call("avd_learn_shared_workspace", ctypes.byref(lay), 10, 5, ctypes.byref(need))
    lay = _hip.make_layout(4, 1, 1024, 1024, 48, 64)
    with pytest.raises(_hip.AvdError, match="multiple of n_sets"):
        _hip.call("avd_learn_shared_workspace", ctypes.byref(lay), 11, 5, ctypes.byref(need))
    _hip.call("avd_learn_shared_workspace", ctypes.byref(lay), 20480, 5, ctypes.byref(need))
    assert 20 * 2**30 < need.value < 40 * 2**30  # BASELINE config 5: ~26 GiB of scratch, fits 288 GB beside the replay ring
    with pytest.raises(_hip.AvdError, match="K %"):
        _hip.call("avd_gemm_bt_bf16", 128, 128, 100, None, 100, None, 100, None, 128, None)


def test_federated_server_keeps_the_reference_class_api():
    """src/server/federated.py:13-16, 18, 69: Server(name, debug_enabled), get_avg_params(system_params),
    get_weighted_avg_params(system_params, weight_sums). No compute here (no GPU): signatures only."""
    import inspect

    from avddpg_amd import federated

    assert list(inspect.signature(federated.Server.__init__).parameters)[:3] == ["self", "name", "debug_enabled"]
    assert list(inspect.signature(federated.Server.get_avg_params).parameters) == ["self", "system_params"]
    assert list(inspect.signature(federated.Server.get_weighted_avg_params).parameters) == ["self", "system_params", "weight_sums"]
    assert "oracle" not in open(federated.__file__).read().split('"""', 2)[2]


def test_learn_update_plan_describes_the_centralized_pipeline_and_single_launch_shapes():
    """avd_learn_update_plan (bench.py described the centralized pipeline with literals of the profiled box): chunks of one
    learn workgroup per CU, at most 32 chunks (the chunk grows instead); every other shape is ONE launch. Without a GPU the CU count
    falls back to 256."""
    import ctypes as C

    cen = _hip.make_layout(20, 5, 320, 160, 64, 64)   # centralized L = 5: S = 4 L, A = L, widths x 1.2 padded
    dec = _hip.make_layout(4, 1, 256, 128, 48, 64)
    ch, n, g = C.c_int(0), C.c_int(0), C.c_int(0)
    _hip.call("avd_learn_update_plan", C.byref(cen), 4096, C.byref(ch), C.byref(n), C.byref(g))
    assert ch.value >= 1 and n.value == (4096 + ch.value - 1) // ch.value and n.value <= 32 and g.value >= 1
    _hip.call("avd_learn_update_plan", C.byref(cen), 100000, C.byref(ch), C.byref(n), C.byref(g))
    assert n.value <= 32 and ch.value * n.value >= 100000
    _hip.call("avd_learn_update_plan", C.byref(dec), 20480, C.byref(ch), C.byref(n), C.byref(g))
    assert (ch.value, n.value, g.value) == (20480, 1, 0)
    with pytest.raises(_hip.AvdError):
        _hip.call("avd_learn_update_plan", C.byref(dec), 0, C.byref(ch), C.byref(n), C.byref(g))


def test_bench_default_run_declares_every_single_gpu_baseline_config():
    """bench.py's --full 1-GPU run must carry BASELINE configs[2] (both federated modes) and configs[4] beside the two configs[1]
    workloads: the keys of also_measured are a module constant, each naming the BASELINE.json entry it measures,
    and the run that emits them is the one with --full and no other flag (tests/test_gpu_bench_ranks.py runs it on the GPU). No GPU,
    no torch here."""
    import importlib.util
    import json
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert set(bench.EXTRA_CONFIGS) == {"config3_interfrl", "config3_nofrl", "config5"}
    configs = json.load(open(os.path.join(root, "BASELINE.json")))["configs"]
    assert "4096 platoons × 10 vehicles" in configs[2] and "hidden=1024" in configs[4]
    assert all("configs[2]" in bench.EXTRA_CONFIGS[k] and "10 vehicles" in bench.EXTRA_CONFIGS[k] for k in ("config3_interfrl", "config3_nofrl"))
    assert "configs[4]" in bench.EXTRA_CONFIGS["config5"] and "1024" in bench.EXTRA_CONFIGS["config5"]
    src = open(os.path.join(root, "bench.py")).read()
    assert "default_run" in src and "--no-extra-configs" in src and 'out.setdefault("also_measured", {}).update(' in src
    assert bench.PRIMARY_MODE == "interfrl"


def test_bench_plain_run_leaves_everything_but_the_headline_to_full(monkeypatch):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times the primary workload only: the second workload, the other BASELINE
    configs, the CPU baseline and the other collective form are measured only with --full, which is off by default. No GPU here."""
    import importlib.util
    import os
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    args = bench.parse()
    assert args.full is False and (args.steps, args.warmup, args.gpus) == (20, 5, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full is True
    src = open(os.path.join(root, "bench.py")).read()
    main_src = src[src.index("def main():"):]
    # each extra measurement is gated on --full
    assert "not args.full or args.no_secondary" in main_src
    assert "default_run = (args.full and" in main_src
    assert "if args.full and world == 1 and not args.no_cpu_baseline:" in main_src
    assert "if args.full and (world > 1 or group is not None)" in src


_PATH_BITS = ("fused_fwd", "fused_delta", "r1", "dual", "act_in_dx")  # AVD_PATH_* of include/avddpg_hip.h, bit 0 upwards
_PATH_QUERY = r"""
import ctypes, sys
from avddpg_amd import _hip
lay = _hip.make_layout(4, 1, 1024, 1024, 48, 64)
flags = ctypes.c_uint(0)
_hip.call("avd_learn_shared_path", ctypes.byref(lay), 2 * 12, 2, ctypes.byref(flags))
print("flags", flags.value)
"""


def _path(S, widths, rows, n_sets=2):
    lay = _hip.make_layout(S, 1, *widths, 64)
    flags = ctypes.c_uint(0)
    _hip.call("avd_learn_shared_path", ctypes.byref(lay), n_sets * rows // 64, n_sets, ctypes.byref(flags))
    assert flags.value < 1 << len(_PATH_BITS)
    return {name for i, name in enumerate(_PATH_BITS) if flags.value >> i & 1}


def test_shared_learner_path_table():
    """avd_learn_shared_path: which form of avd_learn_shared_bf16 a shape takes, decided on the host by the same choose_path the learner
    calls (csrc/wide.hip), no HIP call. A condition that slips sends BASELINE config 5 down the layer-wise chain at about half the speed
    with every oracle test still passing; this table pins the product library's decision. Batches of 64, one action."""
    everything = set(_PATH_BITS)
    for rows in (768, 960, 4096):  # (960 pads to 1024 rows)
        assert _path(4, (1024, 1024, 48), rows) == everything, rows
    # one 256-row chunk per set: below the rank-one chain's two
    assert _path(4, (1024, 1024, 48), 192) == {"fused_fwd", "fused_delta"}
    assert _path(4, (512, 512, 48), 768) == everything - {"act_in_dx"}  # (the action features ride in dx only with four feature blocks)
    assert _path(4, (256, 128, 48), 384) == set()  # the reference widths: second layer not in 512-column blocks
    assert _path(3, (1024, 1024, 48), 768) == set()  # the fused first layer is written for S == 4
    # the action branch must pad to exactly two 32-feature chunks: 1024 + 32 pads to 1088 like 1024 + 48; 1024 + 80 pads to 1152
    assert _path(4, (1024, 1024, 32), 768) == everything
    assert _path(4, (1024, 1024, 80), 768) == {"fused_fwd"}
    with pytest.raises(_hip.AvdError, match="multiples of 64"):
        _path(4, (320, 160, 48), 768)
    lay = _hip.make_layout(4, 1, 1024, 1024, 48, 64)
    with pytest.raises(_hip.AvdError, match="null pointer"):
        _hip.call("avd_learn_shared_path", ctypes.byref(lay), 24, 2, None)


@pytest.mark.parametrize("switch,cleared", [(None, set()), ("AVD_WIDE_DUAL", {"dual"}),
                                            ("AVD_WIDE_FUSED_DELTA", {"fused_delta", "r1", "dual", "act_in_dx"}),
                                            ("AVD_WIDE_FUSED_FWD", set(_PATH_BITS))])
def test_diagnostic_switches_clear_a_path_flag_and_what_rests_on_it(switch, cleared):
    """The diagnostic library's AVD_WIDE_*=0 switches at 1024/1024/48, 768 rows per set: each clears its flag and every flag that rests
    on it, nothing else. One child process per setting (the switches are read once per process); the product library reads none."""
    import subprocess
    import sys

    assert os.path.exists(_hip.DIAG_LIB_PATH), "the diagnostic library is part of build()"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("AVD_WIDE_")}
    env.update(AVDDPG_HIP_LIB=_hip.DIAG_LIB_PATH, PYTHONPATH=root + os.pathsep + env.get("PYTHONPATH", ""))
    if switch:
        env[switch] = "0"
    p = subprocess.run([sys.executable, "-c", _PATH_QUERY], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    flags = int(p.stdout.split("flags")[1])
    assert {name for i, name in enumerate(_PATH_BITS) if flags >> i & 1} == set(_PATH_BITS) - cleared
    if switch:  # the product library holds no switch
        env.pop("AVDDPG_HIP_LIB")
        p = subprocess.run([sys.executable, "-c", _PATH_QUERY], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and int(p.stdout.split("flags")[1]) == (1 << len(_PATH_BITS)) - 1, p.stderr[-2000:]


# ---- the per-agent exact-f32 learner: which kernel a layout gets, and what its entry points refuse on the host -------------------
_LEARN_KERNELS = ("lean", "fast", "cen", "general")  # AVD_LEARN_* of include/avddpg_hip.h, 0 upwards
_REF3, _REF4 = (3, 1, 256, 128, 48), (4, 1, 256, 128, 48)
_CEN3, _CEN5 = (12, 3, 320, 160, 64), (20, 5, 320, 160, 64)
_GEN = (5, 2, 128, 64, 32)
_HP_TWINS = "the HP twins exist for learn_kernel_l only; the diagnostic LEARN_KERNEL / LEARN_GENERAL switches select another kernel"
_HP_WIDTHS = r"a hyperparameter sweep runs the reference widths 256/128/48, A=1, B=64, S in \{3,4\} only \(got %s\)"


def _learn_kernel(dims, hp=0, B=64):
    lay = _hip.make_layout(*dims, B)
    k = ctypes.c_int(-1)
    _hip.call("avd_learn_kernel", ctypes.byref(lay), hp, ctypes.byref(k))
    return _LEARN_KERNELS[k.value]


def test_learn_kernel_table_of_the_product_library():
    """avd_learn_kernel: the kernel avd_learn_f32 / avd_learn_update*_f32 run for a layout, decided on the host by the choose_learner the
    entry points call (csrc/mlp.hip), no HIP call. The product library reads no switch: reference widths -> learn_kernel_l, the
    centralized shapes -> learn_kernel_c, anything else -> learn_kernel_g; the HP twins serve the reference widths only."""
    assert [_learn_kernel(d) for d in (_REF3, _REF4, _CEN3, _CEN5, _GEN)] == ["lean", "lean", "cen", "cen", "general"]
    # next to the table's rows: one width or the action count off the reference / centralized shapes
    assert _learn_kernel((4, 1, 256, 128, 64)) == "general" and _learn_kernel((5, 1, 256, 128, 48)) == "general"
    assert _learn_kernel((16, 4, 320, 160, 64)) == "general" and _learn_kernel((4, 2, 256, 128, 48)) == "general"
    assert _learn_kernel(_REF3, hp=1) == "lean" and _learn_kernel(_REF4, hp=1) == "lean"
    for dims, got in ((_CEN5, "320/160/64, A=5, B=64, S=20"), (_GEN, "128/64/32, A=2, B=64, S=5")):
        with pytest.raises(_hip.AvdError, match=r"failed \(-3\): avd_learn_kernel: " + _HP_WIDTHS % got):
            _learn_kernel(dims, hp=1)
    with pytest.raises(_hip.AvdError, match=r"failed \(-3\): avd_learn_kernel: " + _HP_WIDTHS % "256/128/48, A=1, B=32, S=4"):
        _learn_kernel(_REF4, hp=1, B=32)
    # the shape check comes with it
    with pytest.raises(_hip.AvdError, match=r"failed \(-3\): avd_learn_kernel: batch_size=32; the tile kernels implement B == 64"):
        _learn_kernel(_REF4, B=32)
    with pytest.raises(_hip.AvdError, match=r"failed \(-3\): avd_learn_kernel: .*need 164768 B of LDS"):
        _learn_kernel((24, 6, 320, 160, 64))
    with pytest.raises(_hip.AvdError, match=r"failed \(-1\): avd_learn_kernel: null"):
        _hip.call("avd_learn_kernel", ctypes.byref(_hip.make_layout(*_REF4, 64)), 0, None)


def test_learn_kernel_switches_of_the_diagnostic_library_take_effect_inside_one_process(monkeypatch):
    """The diagnostic library's AVD_LEARN_KERNEL=fast and AVD_LEARN_GENERAL (any value, and it wins over `fast`), read on EVERY call:
    tests/test_gpu_mlp.py and tests/test_gpu_trainer.py set and clear them inside one process. The centralized shapes have no `fast`
    form; with a switch set the HP twins refuse, before they look at the widths. The product library reads neither."""
    assert os.path.exists(_hip.DIAG_LIB_PATH), "the diagnostic library is part of build()"
    shapes = (_REF3, _REF4, _CEN3, _CEN5, _GEN)
    table = {(): ["lean", "lean", "cen", "cen", "general"], ("KERNEL",): ["fast", "fast", "cen", "cen", "general"],
             ("GENERAL",): ["general"] * 5, ("KERNEL", "GENERAL"): ["general"] * 5}
    monkeypatch.delenv("AVD_LEARN_KERNEL", raising=False)
    monkeypatch.delenv("AVD_LEARN_GENERAL", raising=False)
    with _hip.diag_library():
        for setting in ((), ("KERNEL",), ("GENERAL",), ("KERNEL", "GENERAL"), ("KERNEL",), ()):  # set, and cleared again
            for name, value in (("KERNEL", "fast"), ("GENERAL", "0")):
                if name in setting:
                    monkeypatch.setenv("AVD_LEARN_" + name, value)
                else:
                    monkeypatch.delenv("AVD_LEARN_" + name, raising=False)
            assert [_learn_kernel(d) for d in shapes] == table[setting], setting
            if setting:
                for dims in (_REF4, _GEN):
                    with pytest.raises(_hip.AvdError, match=r"failed \(-3\): avd_learn_kernel: " + _HP_TWINS):
                        _learn_kernel(dims, hp=1)
            else:
                assert _learn_kernel(_REF4, hp=1) == "lean"
        monkeypatch.setenv("AVD_LEARN_KERNEL", "lean")  # any other value: the default
        assert _learn_kernel(_REF4) == "lean" and _learn_kernel(_REF4, hp=1) == "lean"
        monkeypatch.setenv("AVD_LEARN_KERNEL", "fast")
        monkeypatch.setenv("AVD_LEARN_GENERAL", "1")
    assert [_learn_kernel(d) for d in shapes] == table[()]  # the product library, both switches still set


_BOGUS = 0x1000  # non-null "device pointers" that nothing reads (one per argument): every call below is refused on the host
_SLABS = ("theta", "stats", "theta_out", "theta_t", "stats_t", "m", "v", "step", "s", "a", "r", "s2")


def _learn_call(entry, lay, n=2, set_mod=0, x_stride=None, hp=(1, 1), **ptrs):
    """Call one of the six learn entry points with non-null pointers everywhere but where `ptrs` says otherwise (name=None)."""
    p = {k: ctypes.c_void_p(_BOGUS * (i + 1)) for i, k in enumerate(_SLABS + ("grads", "losses", "next_state", "next_action", "d_hp"))}
    p.update(ptrs)
    layp = None if lay is None else ctypes.byref(lay)
    update, sweep, act = "update" in entry, "_hp_" in entry, "_act_" in entry
    args = [layp, n] + ([] if update else [set_mod]) + [p[k] for k in _SLABS if update or k not in ("theta_out", "m", "v", "step")]
    args += [2.5] if sweep else ([0.99, 2.5, 1e-4, 1e-3, 0.005] if update else [0.99, 2.5])
    args += [p["grads"], p["losses"]]
    if act:
        args += [p["next_state"], (lay.S if lay is not None else 4) if x_stride is None else x_stride, p["next_action"]]
    if sweep:
        args += [p["d_hp"], *hp]
    _hip.call(entry, *args, None)


# entry point -> the name its messages carry (the scalar update entries share one)
_LEARN_ENTRIES = {"avd_learn_f32": "avd_learn_f32", "avd_learn_update_f32": "avd_learn_update_f32",
                  "avd_learn_update_act_f32": "avd_learn_update_f32", "avd_learn_hp_f32": "avd_learn_hp_f32",
                  "avd_learn_update_hp_f32": "avd_learn_update_hp_f32", "avd_learn_update_act_hp_f32": "avd_learn_update_act_hp_f32"}


@pytest.mark.parametrize("entry", sorted(_LEARN_ENTRIES))
def test_learn_entry_points_refuse_on_the_host_before_any_hip_call(entry):
    """Everything the six learn entry points refuse before their first HIP call, one fault per call, with status and message: the
    contract the entry points keep whichever way their host code is arranged (no GPU here: a call that got past its checks would
    fail with a HIP error instead)."""
    who, update, sweep, act = _LEARN_ENTRIES[entry], "update" in entry, "_hp_" in entry, "_act_" in entry
    ref, refuse = _hip.make_layout(*_REF4, 64), lambda code, msg: pytest.raises(_hip.AvdError, match=rf"failed \({code}\): {msg}")
    with refuse(-1, f"{entry}: next_state / x_stride" if act else f"{who}: null layout"):
        _learn_call(entry, None)
    with refuse(-1, f"{who}: n_agents=0"):
        _learn_call(entry, ref, n=0)
    with refuse(-1, f"{who}: n_agents=-3"):
        _learn_call(entry, ref, n=-3)
    if not update:
        with refuse(-1, f"{who}: n_agents=2 set_mod=-1"):
            _learn_call(entry, ref, set_mod=-1)
    for name in _SLABS + ("grads",):
        if update or name not in ("theta_out", "m", "v", "step"):
            with refuse(-1, f"{who}: null pointer"):
                _learn_call(entry, ref, **{name: None})
    if update:
        with refuse(-1, f"{who}: theta_out must not alias theta"):
            _learn_call(entry, ref, theta=ctypes.c_void_p(0x2000), theta_out=ctypes.c_void_p(0x2000))
    if act:
        for fault in (dict(x_stride=3), dict(next_state=None), dict(next_action=None)):
            with refuse(-1, f"{entry}: next_state / x_stride"):
                _learn_call(entry, ref, **fault)
    if sweep:
        for fault in (dict(d_hp=None), dict(hp=(0, 1)), dict(hp=(1, 0)), dict(n=6, hp=(2, 2))):
            with refuse(-1, rf"{who}: d_hp=.* \(the count must be a multiple of n_groups x set_block\)"):
                _learn_call(entry, ref, **fault)
    # shapes
    with refuse(-3, rf"{who}: need S <= 64, A <= 16, H1 and Ha multiples of 16, H2 a multiple of 32 and <= 256 \(got S=4 A=1 H1=256 H2=288 "
                    r"Ha=48\); pad the widths with zero units"):
        _learn_call(entry, _hip.make_layout(4, 1, 256, 288, 48, 64))
    with refuse(-3, rf"{who}: need S <= 64.*got S=12 A=3 H1=307 H2=153 Ha=57"):
        _learn_call(entry, _hip.make_layout(12, 3, 307, 153, 57, 64))
    sweep_who = "avd_learn_update(_act)?_hp_f32" if act else who  # (the act twin's width refusal has carried either name)
    with refuse(-3, f"{sweep_who}: " + _HP_WIDTHS % "256/128/48, A=1, B=32, S=4" if sweep else
                    f"{who}: batch_size=32; the tile kernels implement B == 64"):
        _learn_call(entry, _hip.make_layout(*_REF4, 32))
    with refuse(-3, f"{sweep_who}: " + _HP_WIDTHS % "320/160/64, A=6, B=64, S=24" if sweep else
                    rf"{who}: S=24 A=6 H1=320 H2=160 Ha=64 need 164768 B of LDS per 64-row tile \(> 160 KiB\)"):
        _learn_call(entry, _hip.make_layout(24, 6, 320, 160, 64, 64))
    if sweep:  # the HP twins exist at the reference widths only
        for dims, got in ((_GEN, "128/64/32, A=2, B=64, S=5"), (_CEN3, "320/160/64, A=3, B=64, S=12"), ((5, 1, 256, 128, 48), "256/128/48, A=1, B=64, S=5")):
            with refuse(-3, f"{sweep_who}: " + _HP_WIDTHS % got):
                _learn_call(entry, _hip.make_layout(*dims, 64))


def test_learn_update_plan_refuses_null_arguments_and_runs_no_shape_check():
    """avd_learn_update_plan, the seventh entry of the per-agent learner: null arguments and n_agents <= 0 are refused; a layout the
    learner itself would refuse is still described (one launch)."""
    import ctypes as C

    lay, out = _hip.make_layout(*_CEN5, 64), [C.c_int(0) for _ in range(3)]
    for args in ((None, 8, *map(C.byref, out)), (C.byref(lay), 8, None, C.byref(out[1]), C.byref(out[2])),
                 (C.byref(lay), 8, C.byref(out[0]), None, C.byref(out[2])), (C.byref(lay), 8, C.byref(out[0]), C.byref(out[1]), None),
                 (C.byref(lay), -1, *map(C.byref, out))):
        with pytest.raises(_hip.AvdError, match=rf"failed \(-1\): avd_learn_update_plan: null / n_agents={args[1]}"):
            _hip.call("avd_learn_update_plan", *args)
    for dims, B in (((24, 6, 320, 160, 64), 64), (_CEN5, 32), ((4, 1, 256, 288, 48), 64)):
        _hip.call("avd_learn_update_plan", C.byref(_hip.make_layout(*dims, B)), 100, *map(C.byref, out))
        assert [o.value for o in out] == [100, 1, 0]
