"""CPU checks of the evaluator rollout entry point (avd_eval_rollout_f32, csrc/eval.hip): every argument is checked on the
host before any HIP call, so a bad call returns AVD_E_INVALID with a message and touches no device. Every call below fails
one check; none reaches a launch."""
import ctypes as C

import pytest

from avddpg_amd import _hip

AVD_E_INVALID = -1
FAKE = C.c_void_p(0x1000)  # a non-null "device pointer": the checks only test it for NULL, nothing dereferences it on the host


def _args(**kw):
    """Valid arguments of a decentralized L = 5 rollout (reference widths), with `kw` overriding some."""
    a = dict(lay=C.byref(_hip.make_layout(4, 1, 256, 128, 48, 64)), consts=FAKE, R=8, L=5, M=5, T=600, theta=FAKE, stats=FAKE,
             n_sets=40, set_base=FAKE, x0=FAKE, prev_a0=FAKE, leader=FAKE, n_start=1, start_idx=FAKE, high=2.5, lo=-2.5, hi=2.5,
             sample_rate=0.1, counters=FAKE, n_trace=0, trace_idx=None, tr_states=None, tr_actions=None, tr_jerks=None, stream=None)
    a.update(kw)
    return list(a.values())


def _rc_and_message(**kw):
    lib = _hip.lib()
    rc = lib.avd_eval_rollout_f32(*_args(**kw))
    return rc, lib.avd_last_error().decode()


@pytest.mark.parametrize("kw,match", [
    (dict(L=0, M=0), "L=0 (L must be 1..16)"),
    (dict(L=17, M=17), "L=17 (L must be 1..16)"),
    (dict(M=2), "M=2 (M must be L=5"),
    (dict(M=0), "M=0 (M must be L=5"),
    (dict(T=0), "T=0 (both must be >= 1)"),
    (dict(R=0), "R=0 T=600 (both must be >= 1)"),
    (dict(R=-3), "R=-3"),
    (dict(lay=None), "null layout or constants"),
    (dict(consts=None), "null layout or constants"),
    (dict(theta=None), "null pointer"),
    (dict(stats=None), "null pointer"),
    (dict(set_base=None), "null pointer"),
    (dict(x0=None), "null pointer"),
    (dict(prev_a0=None), "null pointer"),
    (dict(leader=None), "null pointer"),
    (dict(start_idx=None), "null pointer"),
    (dict(counters=None), "null pointer"),
    (dict(n_trace=2), "n_trace=2 needs trace_idx and the three trace buffers"),
    (dict(n_trace=1, trace_idx=FAKE, tr_states=FAKE, tr_actions=FAKE), "n_trace=1 needs trace_idx"),
    (dict(n_trace=-1), "n_trace=-1"),
    (dict(n_sets=4), "n_sets=4 n_start=1"),
    (dict(n_start=0), "n_sets=40 n_start=0"),
    (dict(sample_rate=0.0), "sample_rate=0"),
])
def test_bad_arguments_are_refused_before_any_hip_call(kw, match):
    rc, msg = _rc_and_message(**kw)
    assert rc == AVD_E_INVALID and msg.startswith("avd_eval_rollout_f32: ") and match in msg, (rc, msg)


def test_layout_must_fit_the_platoon():
    # centralized (M = 1) needs A = L actions and S <= 4L; decentralized Model A / B S <= 4, A = 1
    rc, msg = _rc_and_message(M=1)  # A = 1 layout for a 5-vehicle centralized platoon
    assert rc == AVD_E_INVALID and "does not fit L=5 M=1" in msg
    cen = C.byref(_hip.make_layout(12, 3, 320, 160, 64, 64))
    rc, msg = _rc_and_message(lay=cen, L=3, M=3)
    assert rc == AVD_E_INVALID and "layout S=12 A=3 does not fit L=3 M=3" in msg


def test_python_binding_raises_with_the_message():
    with pytest.raises(_hip.AvdError, match=r"avd_eval_rollout_f32 failed \(-1\): .*L=99"):
        _hip.call("avd_eval_rollout_f32", *_args(L=99, M=99))
