"""The named state FilterEngine.run leaves for finish_pending (nfdpf.engine.Pending / Verify): its
twelve fields in the positional order bench.py indexes, and the readers that take it by name.  CPU
only: the states are built by hand, no device and no library call."""
import pytest

from nfdpf import _lib as L
from nfdpf.engine import FilterEngine, Pending, ShardInfo, Verify


def _pendings():
    decided = Pending(None, None, ShardInfo(), 100, "res", None, Verify("flags", "obs", None, None), True, True,
                      None, None, [])
    checked = Pending("parts", "tot", ShardInfo(), 100, "res", None, Verify(None, "obs", [0, 0, 1], "lease"), True,
                      False, None, "gates", [])
    return decided, checked


def test_pending_is_twelve_named_fields_in_the_positional_order():
    assert Pending._fields == ("parts", "tot", "shard", "N", "res", "split_dev", "verify", "was_pass", "decided",
                               "plan", "gates", "stage")
    assert Verify._fields == ("flags_dev", "obs", "flags_host", "lease")
    for p in _pendings():
        assert len(p) == 12
        assert p[6] is p.verify and p[6][0] is p.verify.flags_dev
        assert p[0] is p.parts and p[10] is p.gates and p[11] is p.stage
    decided, checked = _pendings()
    assert decided[8] and not checked[8]
    assert decided.stage is not checked.stage  # (staged copies are per pass)


def test_pending_pass_state_by_name():
    decided, checked = _pendings()
    with pytest.raises(L.NfdpfError):
        FilterEngine.pending_pass_state(decided)
    st = FilterEngine.pending_pass_state(checked)
    assert st == dict(gates="gates", obs="obs", parts="parts", flags=(0, 0, 1))


def test_arm_flags_clears_the_completion_word_only_where_mapped():
    decided, checked = _pendings()
    FilterEngine.arm_flags(decided)  # (flags in device memory: nothing to arm)
    FilterEngine.arm_flags(checked)
    assert checked.verify.flags_host == [0, 0, 0]
    assert FilterEngine.wait_flags(decided) is False


# ---- finish_pending on hand-built states whose flags are already on the host (synced=True) -------------

def _eng():
    from nfdpf.engine import FilterConfig
    return FilterEngine(FilterConfig(N=100, NF_dyn=True, NF_cond=True, measurement="cos", resampler="soft"), models=None)


def _state(flags, *, was_pass=True, decided=False, plan=None, gates=None, flags_dev=None, stage=None):
    import types
    res = types.SimpleNamespace(obs_likelihood=None)
    verify = Verify(flags_dev, "obs", None if flags_dev is not None else list(flags), None)
    return Pending("parts", None, ShardInfo(), 100, res, None, verify, was_pass, decided, plan, gates,
                   [] if stage is None else stage)


def test_finish_pending_ok_fired_and_decided():
    e = _eng()
    p = _state([0, 0, 1])
    assert e.finish_pending(p, synced=True) and e.last_verify == "ok" and p.res.obs_likelihood == "obs"
    p = _state([2, 0, 1])
    assert not e.finish_pending(p, synced=True) and e.last_verify == "fired" and p.res.obs_likelihood is None
    p = _state([2, 0, 1], decided=True)  # (the gates were decided inside the launch: only faults count)
    assert e.finish_pending(p, synced=True) and e.last_verify == "ok" and p.res.obs_likelihood == "obs"


def test_finish_pending_plan_miss_takes_the_actual_gates():
    import numpy as np
    import torch
    e = _eng()
    p = _state([1, 0, 1], plan=np.array([0, 1, 0], np.int32), gates=torch.tensor([0, 1, 1], dtype=torch.int32))
    assert not e.finish_pending(p, synced=True) and e.last_verify == "fired"
    assert e._plan.tolist() == [0, 1, 1]


def test_finish_pending_faults():
    e = _eng()
    with pytest.warns(RuntimeWarning, match="timed out"):
        assert not e.finish_pending(_state([0, 3, 1]), synced=True)
    assert e.last_verify == "fault" and e.pass_disabled
    e = _eng()
    with pytest.raises(L.NfdpfError, match="3 wave hand-off"):  # (step launches: the outputs are invalid)
        e.finish_pending(_state([0, 3, 1], was_pass=False), synced=True)
    assert not e.pass_disabled


def test_finish_pending_reads_the_staged_copy_once_synced():
    import torch
    e = _eng()
    dev = torch.tensor([5, 0, 1], dtype=torch.int32)   # (what a later replay may already have overwritten)
    p = _state(None, flags_dev=dev, stage=[torch.tensor([0, 0, 1], dtype=torch.int32)])
    assert e.finish_pending(p, synced=True) and e.last_verify == "ok"
    p = _state(None, flags_dev=dev)  # (nothing staged: the device flags themselves)
    assert not e.finish_pending(p, synced=True) and e.last_verify == "fired"
