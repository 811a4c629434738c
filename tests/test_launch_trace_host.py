"""Launch-trace pin of the NAFNet executor (no GPU): the executor runs on CPU tensors with _lib._call replaced by a
recorder, and the sequence of launches -- every entry point, every scalar, every tensor operand by identity, dtype and
size -- is compared with tests/golden/launch_trace.json.

The golden file was recorded with this module from the commit BEFORE the executor was restructured around BlockPlan
(`python tests/test_launch_trace_host.py OUT.json`, run in a checkout of that commit).  It pins behaviour, so it is
never regenerated from the code under test: when a digest differs, dump both traces (trace_of) and fix the executor.
"""
import hashlib
import json
import os
import sys
from collections import Counter

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from lowlight_image_enhancement_amd import _lib  # noqa: E402
from lowlight_image_enhancement_amd.nafnet import NAFNet, NAFNetLocal  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.json")

NETS = {
    1: (dict(width=32, enc_blk_nums=[2, 2], middle_blk_num=2, dec_blk_nums=[2, 2]), (1, 3, 64, 64)),
    2: (dict(width=32, enc_blk_nums=[1, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1]), (1, 3, 256, 256)),
    3: (dict(width=16, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1]), (2, 3, 50, 46)),
    4: (dict(width=4, enc_blk_nums=[1], middle_blk_num=1, dec_blk_nums=[1]), (1, 3, 16, 16)),
    5: (dict(width=8, enc_blk_nums=[1], middle_blk_num=1, dec_blk_nums=[1]), (1, 3, 16, 16)),
}
SWITCHES = ("fuse_ln_fwd", "group_wgrad", "sg_rc", "sg_rc_wg", "fuse_ffn", "fuse_ffn_rows", "sca_fold", "ln_wg",
            "fuse_c1dw", "fuse_c1dw_tile")
LOCAL = (dict(width=32, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1]), (1, 3, 32, 32), (1, 3, 64, 64))


class Recorder:
    """Stands in for _lib._call(name, args): records [name, arg...], a tensor as [index, dtype, numel] with the index
    the first-seen number of its (storage address, storage offset).  Every tensor seen stays referenced, so no address
    is reused within a run.  fail_on: raise NBPError at the first launch of that name (recorded first)."""

    def __init__(self, fail_on=None):
        self.trace, self.ids, self.alive, self.fail_on = [], {}, [], fail_on

    def _arg(self, a):
        if not isinstance(a, torch.Tensor):
            return a
        self.alive.append(a)
        key = (a.untyped_storage().data_ptr(), a.storage_offset())
        return [self.ids.setdefault(key, len(self.ids)), str(a.dtype), a.numel()]

    def __call__(self, name, args):
        self.trace.append([name] + [self._arg(a) for a in args])
        if name == self.fail_on:
            self.fail_on = None
            raise _lib.NBPError(f"nbp_{name} failed (injected)")
        return 0

    def hook(self, stage):
        self.trace.append(["hook", stage.name, stage.lo, stage.hi])


def make_net(case, off=()):
    cfg, shape = NETS[case]
    torch.manual_seed(0)
    net = NAFNet(img_channel=3, **cfg)
    for name in off:
        assert getattr(net, name) is True, name
        setattr(net, name, False)
    return net, torch.zeros(shape)


def run(net, x, precision, save, rec, hook=False, between=None):
    """exec_forward, then (save) exec_backward on zero gradients; `between` runs after the forward."""
    real, _lib._call = _lib._call, rec
    try:
        out, tape = net.exec_forward(x, save, precision=precision)
        if between is not None:
            between()
        if save:
            net.exec_backward(tape, torch.zeros_like(out), torch.zeros_like(net.flat.data), need_dx=True,
                              hook=rec.hook if hook else None)
    finally:
        _lib._call = real
    return rec.trace


def summary(trace):
    canon = json.dumps(trace, separators=(",", ":"), sort_keys=True)
    return {"launches": len(trace), "names": dict(sorted(Counter(t[0] for t in trace).items())),
            "sha256": hashlib.sha256(canon.encode()).hexdigest()}


def _cases():
    cases = {}
    for case, precs in ((1, ("fp32", "fp16", "bf16")), (2, ("fp32", "fp16", "bf16")), (3, ("fp32", "fp16", "bf16")),
                        (4, ("fp32",)), (5, ("fp32", "fp16", "bf16"))):
        for p in precs:
            for save in ((True, False) if case <= 3 else (True,)):
                cases[f"case{case}-{p}-{'save' if save else 'nosave'}"] = dict(case=case, precision=p, save=save)
    cases["case1-fp16-save-hook"] = dict(case=1, precision="fp16", save=True, hook=True)
    for s in SWITCHES:
        cases[f"case2-fp16-save-no-{s}"] = dict(case=2, precision="fp16", save=True, off=(s,))
    cases["case1-fp16-save-no-ffn_rows_pre"] = dict(case=1, precision="fp16", save=True, off=("ffn_rows_pre",))
    cases["local-fp16-nosave"] = dict(local=True)
    return cases


CASES = _cases()


def trace_of(name):
    spec = dict(CASES[name])
    if spec.pop("local", False):
        cfg, train, shape = LOCAL
        torch.manual_seed(0)
        net = NAFNetLocal(img_channel=3, train_size=train, **cfg)
        assert any(net.local_blocks(shape[2], shape[3]).values())
        return run(net, torch.zeros(shape), "fp16", False, Recorder())
    net, x = make_net(spec.pop("case"), spec.pop("off", ()))
    return run(net, x, spec["precision"], spec["save"], Recorder(), hook=spec.get("hook", False))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_lists_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_trace_matches_the_recorded_one(golden, name):
    got, want = summary(trace_of(name)), golden[name]
    assert got["launches"] == want["launches"]
    assert got["names"] == want["names"]
    assert got["sha256"] == want["sha256"]


def test_the_cases_reach_every_entry_point_the_executor_launches(golden):
    import re
    src = open(os.path.join(ROOT, "lowlight_image_enhancement_amd", "nafnet.py")).read()
    named = set(re.findall(r'\bcall\("(\w+)"', src))
    reached = set().union(*(g["names"] for g in golden.values()))
    assert len(named) > 40 and named <= reached, sorted(named - reached)


def test_backward_obeys_the_tape_not_the_live_switches(golden):
    """Switches flipped between a forward and its backward change nothing: the backward runs the recorded plan."""
    net, x = make_net(2)

    def flip():
        for s in ("sg_rc_wg", "fuse_ffn_rows", "ln_wg", "sca_fold"):
            setattr(net, s, False)
    got = summary(run(net, x, "fp16", True, Recorder(), between=flip))
    assert got == golden["case2-fp16-save"]


def test_error_inside_a_grouped_level_resets_the_library_and_leaks_no_state(golden):
    net, x = make_net(1)
    rec = Recorder(fail_on="ffn_rows_bwd")
    with pytest.raises(_lib.NBPError, match="injected"):
        run(net, x, "fp16", True, rec)
    at = [i for i, t in enumerate(rec.trace) if t[0] == "ffn_rows_bwd"]
    assert len(at) == 1
    assert rec.trace[at[0] + 1:] == [["wgrad_group", 0], ["grad_reduce_flush", 1]]
    assert net._active is None
    assert summary(run(net, x, "fp16", True, Recorder())) == golden["case1-fp16-save"]


if __name__ == "__main__":  # record the golden file: only ever from the commit before the restructuring (see above)
    with open(sys.argv[1], "w") as f:
        json.dump({name: summary(trace_of(name)) for name in CASES}, f, indent=1, sort_keys=True)
        f.write("\n")
