"""HBM-resident SID dataset, host side (no GPU): the residency plan (distinct frames, byte budget, long-frame
check), the crop descriptors against the reference's draws (oracle/sid_input.py), the host validation that guards
the gather launch, pickling without device state, and the loader rule (num_workers == 0)."""
import pickle

import numpy as np
import pytest
import torch

from oracle import sid_input as osid
from sid_resident_fixtures import (LONG_OF, LONG_SHAPES, SHORT_SHAPES, gold_disk_backend, gold_opt,
                                   write_shared_long_set)


def _frame_bytes(shapes):
    return sum(h * w * 3 * 2 for h, w in shapes)


def test_plan_stores_a_shared_long_frame_once(tmp_path):
    from lowlight_image_enhancement_amd.data import SonySIDResidentDataset, plan_resident
    opt, _ = write_shared_long_set(str(tmp_path))
    ds = SonySIDResidentDataset(opt)
    plan = ds.plan
    assert len(plan.frames) == 4 + 2 and len(set(plan.frames)) == 6
    assert sorted(plan.frames) == sorted([("short", k) for k in SHORT_SHAPES] + [("long", k) for k in LONG_SHAPES])
    want = {**{("short", k): v for k, v in SHORT_SHAPES.items()}, **{("long", k): v for k, v in LONG_SHAPES.items()}}
    assert [plan.shapes[i] for i in range(6)] == [want[k] for k in plan.frames]
    assert list(plan.nbytes) == [h * w * 3 * 2 for h, w in plan.shapes]
    assert plan.total_bytes == _frame_bytes(list(SHORT_SHAPES.values()) + list(LONG_SHAPES.values()))
    assert len(plan.pairs) == 4 and len(ds) == 8
    for (si, li), s in zip(plan.pairs, SHORT_SHAPES):
        assert plan.frames[si] == ("short", s) and plan.frames[li] == ("long", LONG_OF[s])
    assert len({li for _, li in plan.pairs[:3]}) == 1 and plan.pairs[3][1] != plan.pairs[0][1]
    # the pure function on the same entries and header shapes
    shapes = {k: (*want[k], 3) for k in want}
    assert plan_resident(ds.entries, shapes, 8, "train", True) == plan
    with pytest.raises(ValueError, match=r"Expected 3-channel image, got shape \(16, 31, 4\)"):
        plan_resident(ds.entries, {**shapes, ("long", "la.png"): (16, 31, 4)}, 8, "train", True)


def test_plan_budget_is_checked_before_any_decode(tmp_path, monkeypatch):
    """One byte short raises, naming the need and the budget; nothing is decoded: the IDAT streams are corrupt (the
    headers are fine), and the native decoder is not called at all."""
    from lowlight_image_enhancement_amd.data import SonySIDResidentDataset, sony_sid_resident_dataset as mod
    calls = []
    real = mod.host_call
    monkeypatch.setattr(mod, "host_call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    opt, _ = write_shared_long_set(str(tmp_path), corrupt_idat=True)
    need = _frame_bytes(list(SHORT_SHAPES.values()) + list(LONG_SHAPES.values()))
    with pytest.raises(ValueError, match=rf"needs {need} bytes .* budget of {need - 1} bytes"):
        SonySIDResidentDataset(dict(opt, resident={"max_bytes": need - 1}))
    ds = SonySIDResidentDataset(dict(opt, resident={"max_bytes": need, "decode_threads": 2}))
    assert ds.plan.total_bytes == need and ds.decode_threads == 2 and ds._resident is None
    ds[0]
    assert calls == []
    from lowlight_image_enhancement_amd.data.sony_sid_lmdb_dataset import _load_png_uint16
    with pytest.raises(ValueError):  # the fixture really cannot be decoded
        _load_png_uint16(ds._fetch_bytes("s0.png", client_key="short"))


@pytest.mark.parametrize("phase,random_crop", [("train", True), ("train", False), ("val", True)])
def test_plan_rejects_a_long_frame_smaller_than_the_window(tmp_path, phase, random_crop):
    from lowlight_image_enhancement_amd.data import SonySIDResidentDataset
    opt, _ = write_shared_long_set(str(tmp_path), long_shapes={"lb.png": (8, 12)}, phase=phase,
                                   random_crop=random_crop)  # s3 is 10 x 10
    with pytest.raises(ValueError, match=r"Long-exposure image \(8, 12, 3\) is smaller than the crop window"):
        SonySIDResidentDataset(opt)
    # a centre crop that stays inside the smaller long frame is accepted, as by SonySIDLMDBDataset
    ok, _ = write_shared_long_set(str(tmp_path), long_shapes={"lb.png": (8, 12)}, random_crop=False, patch_size=4)
    assert len(SonySIDResidentDataset(ok).plan.frames) == 6


@pytest.mark.parametrize("backend,phase,random_crop", [("lmdb", "train", True), ("disk", "train", False),
                                                       ("disk", "val", True)])
def test_descriptors_draw_the_reference_windows(backend, phase, random_crop):
    """The cases of test_dataset_samples_match_reference_arithmetic: with seed 123 the (top, left) sequence over
    range(len(ds)) is the oracle's crop_window drawn from default_rng(123), and equals SonySIDLMDBDataset's."""
    from lowlight_image_enhancement_amd.data import SonySIDLMDBDataset, SonySIDResidentDataset
    kw = dict(phase=phase, random_crop=random_crop, return_metadata=True)
    if backend == "disk":
        kw["io_backend"] = gold_disk_backend()
    if phase == "val":
        kw.update(subset="val_small", samples_per_pair=1)
    ds = SonySIDResidentDataset(gold_opt(**kw))
    base = SonySIDLMDBDataset(gold_opt(**kw))
    assert len(ds) == len(base) and len(ds.plan.frames) == 2 and ds.plan.shapes == ((64, 64), (64, 64))
    rng = np.random.default_rng(123)
    for i in range(len(ds)):
        smp, ref = ds[i], base[i]
        win = osid.crop_window(rng, 64, 64, 24, phase, random_crop)
        assert smp["desc"].dtype == torch.int32 and smp["desc"].tolist() == [0, 1, *win]
        assert tuple(ref["lq_u16"].shape) == (win[2], win[3], 3)
        assert "lq_u16" not in smp and "gt_u16" not in smp
        assert set(smp) - {"desc"} == set(ref) - {"lq_u16", "gt_u16"}
        assert torch.equal(smp["expo_ratio"], ref["expo_ratio"]) and smp["metadata"] == ref["metadata"]
        for k in ("pair_id", "lq_path", "gt_path", "key"):
            assert smp[k] == ref[k]
    if phase == "train" and random_crop:
        assert len({tuple(ds[i]["desc"].tolist()) for i in range(len(ds))}) > 1
    with pytest.raises(ValueError, match="Patch size 65 exceeds"):
        SonySIDResidentDataset(gold_opt(patch_size=65))[0]


def test_host_validation_of_descriptors(tmp_path):
    """What crop_batch checks before it launches (the kernel's clamps are the second line, not the first)."""
    from lowlight_image_enhancement_amd.data import SonySIDResidentDataset
    opt, _ = write_shared_long_set(str(tmp_path))
    ds = SonySIDResidentDataset(opt)
    s0, la = ds.plan.frames.index(("short", "s0.png")), ds.plan.frames.index(("long", "la.png"))  # 12 x 20, 16 x 31
    good = [[s0, la, 0, 0, 8, 8], [s0, la, 4, 12, 8, 8]]
    assert ds.check_descriptors(torch.tensor(good, dtype=torch.int32)).tolist() == good
    for bad in ([s0, 6, 0, 0, 8, 8], [-1, la, 0, 0, 8, 8],              # frame index out of range
                [s0, la, 5, 0, 8, 8], [s0, la, 0, 13, 8, 8],             # past the bottom / right of the short frame
                [la, s0, 8, 0, 8, 8],                                    # inside the first frame, outside the second
                [s0, la, -1, 0, 8, 8], [s0, la, 0, -1, 8, 8],
                [s0, la, 0, 0, 8, 4], [s0, la, 0, 0, 0, 8],              # two window sizes in a batch; empty window
                [s0, la, 2 ** 31 - 8, 0, 8, 8]):
        with pytest.raises(ValueError):
            ds.check_descriptors(torch.tensor([good[0], bad], dtype=torch.int64))
    for bad in (torch.zeros(0, 6, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32),
                torch.zeros(6, dtype=torch.int32), torch.zeros(1, 6)):
        with pytest.raises(ValueError):
            ds.check_descriptors(bad)
    with pytest.raises(ValueError):  # raised before the build: no device is touched
        ds.crop_batch(torch.tensor([[s0, la, 5, 0, 8, 8]], dtype=torch.int32), torch.ones(1))
    assert ds._resident is None


def test_pickled_copy_carries_no_device_state():
    from lowlight_image_enhancement_amd.data import SonySIDResidentDataset
    ds = SonySIDResidentDataset(gold_opt())

    class DeviceState:  # stands in for the resident tensors: refuses to be pickled
        frames = [torch.zeros(3)]

        def __reduce__(self):
            raise AssertionError("the device state must not be pickled")

    ds._resident = DeviceState()
    first = ds[0]["desc"].tolist()
    blob = pickle.dumps(ds)
    assert ds._resident is not None  # the live object keeps its state
    copy = pickle.loads(blob)
    assert copy._resident is None and copy.file_client is None and copy.plan == ds.plan
    assert not any(torch.is_tensor(v) for v in vars(copy).values())
    assert len(blob) < 8192
    assert len(copy) == len(ds) and copy[0]["desc"].tolist()[:2] == first[:2]
    with pytest.raises(RuntimeError):
        copy.build()


def test_loader_uses_no_workers_for_the_resident_dataset():
    from lowlight_image_enhancement_amd.data import SonySIDLMDBDataset, SonySIDResidentDataset, create_dataloader
    opt = {"phase": "train", "batch_size_per_gpu": 2, "num_worker_per_gpu": 4}
    dl = create_dataloader(SonySIDResidentDataset(gold_opt(samples_per_pair=4)), opt, num_gpu=1, seed=0)
    assert dl.num_workers == 0 and dl.batch_size == 2 and dl.drop_last
    assert create_dataloader(SonySIDResidentDataset(gold_opt()), opt, num_gpu=2, dist=True).num_workers == 0
    batches = list(dl)
    assert len(batches) == 2 and batches[0]["desc"].shape == (2, 6) and batches[0]["expo_ratio"].shape == (2, 1, 1, 1)
    # the uint16 dataset keeps what the options ask for
    base = create_dataloader(SonySIDLMDBDataset(gold_opt()), opt, num_gpu=1, seed=0)
    assert base.num_workers == 4
