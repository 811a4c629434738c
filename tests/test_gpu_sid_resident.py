"""HBM-resident SID dataset on the device: nbp_sid_crop_to_float (sid_resident.hip) bitwise against the oracle's
numpy float32 arithmetic on host-cropped arrays (oracle/sid_input.py) and against nbp_sid_to_float on the same crops;
SonySIDResidentDataset end to end through create_dataloader and CUDAPrefetcher against the SonySIDLMDBDataset path.

The descriptors here are all valid: the kernel's clamps (frame index to [0, F), source pixel to the frame) are a
second line behind crop_batch's host validation and are checked by reading them, never by launching a bad one.
"""
import numpy as np
import pytest
import torch

from oracle import sid_input as osid
from sid_resident_fixtures import gold_disk_backend, gold_opt, read_gold, write_shared_long_set

pytestmark = pytest.mark.gpu

RATIOS = [1.0, 10.0, 100.0, 250.0, 300.0, 0.5]  # those of test_sid_to_float_bitwise_vs_oracle
SHAPES = [(37, 53), (64, 64), (17, 300), (40, 300), (64, 64)]  # frames 0-2 short, 3-4 long
BUDGET = {"max_bytes": 1 << 20}  # explicit, so that the tests do not depend on what else uses the device


@pytest.fixture(scope="module")
def frames(dev):
    """Host arrays and their device copies, pointer table and sizes: made once, never written."""
    rng = np.random.default_rng(2848)
    host = [rng.integers(0, 65536, (h, w, 3)).astype(np.uint16) for h, w in SHAPES]
    for a in host:  # the extremes and 0.1 at both corners of every frame
        a[0, 0] = [0, 65535, 6553]
        a[-1, -1] = [65535, 6553, 0]
    device = [torch.from_numpy(a.view(np.int16)).to(dev) for a in host]
    ptrs = torch.tensor([t.data_ptr() for t in device], dtype=torch.int64).to(dev)
    hw = torch.tensor(SHAPES, dtype=torch.int32).to(dev)
    return host, device, ptrs, hw


def _check(frames, dev, desc, ratios, h, w):
    from lowlight_image_enhancement_amd._lib import call
    host, _, ptrs, hw = frames
    B = len(desc)
    d = torch.tensor(desc, dtype=torch.int32).to(dev)
    r = torch.tensor(ratios, dtype=torch.float32, device=dev)
    lq, sraw, lraw = (torch.full((B, 3, h, w), -7.0, device=dev) for _ in range(3))
    call("sid_crop_to_float", ptrs, hw, d, r, B, len(host), h, w, lq, sraw, lraw)
    s_crop = np.stack([host[si][t:t + h, l_:l_ + w] for si, _, t, l_ in desc])
    l_crop = np.stack([host[li][t:t + h, l_:l_ + w] for _, li, t, l_ in desc])
    assert s_crop.shape == l_crop.shape == (B, h, w, 3)
    lq2, sraw2, lraw2 = (torch.empty(B, 3, h, w, device=dev) for _ in range(3))
    s16, l16 = (torch.from_numpy(a.view(np.int16)).to(dev) for a in (s_crop, l_crop))
    call("sid_to_float", s16, l16, r, B, h, w, lq2, sraw2, lraw2)
    assert torch.equal(lq, lq2) and torch.equal(sraw, sraw2) and torch.equal(lraw, lraw2)
    got = [t.cpu().numpy() for t in (lq, sraw, lraw)]
    for b in range(B):
        ref = osid.getitem_arrays(s_crop[b], l_crop[b], ratios[b], (0, 0, h, w))
        assert np.array_equal(got[0][b], ref["lq"]), b
        assert np.array_equal(got[1][b], ref["short_raw"]), b
        assert np.array_equal(got[2][b], ref["long_raw"]), b


def test_crop_kernel_bitwise_vs_oracle(frames, dev):
    desc = [(0, 3, 0, 0),       # top = left = 0; short 53 wide, long 300 wide
            (0, 3, 21, 29),     # flush with the short frame's bottom-right corner; odd left; the same long frame
            (1, 4, 48, 40),     # flush with the corner of both frames
            (2, 3, 1, 275),     # odd left, last row of the 17-row frame
            (1, 4, 5, 7),
            (3, 3, 24, 276)]    # one frame named as short and as long, flush with its corner
    _check(frames, dev, desc, RATIOS, 16, 24)


def test_crop_kernel_whole_frame_window(frames, dev):
    """The val shape: the window is the frame (more than one block along W)."""
    _check(frames, dev, [(2, 3, 0, 0)], [250.0], 17, 300)
    _check(frames, dev, [(3, 3, 0, 0)], [0.5], 40, 300)


def test_crop_kernel_one_pixel_window(frames, dev):
    _check(frames, dev, [(0, 3, 0, 0), (0, 3, 36, 52), (1, 4, 63, 63), (2, 3, 16, 299)], RATIOS[:4], 1, 1)


def test_crop_kernel_every_uint16_value(dev):
    """The kernel forms u / 65535 from a reciprocal and one correction step: every one of the 65 536 inputs must
    give numpy's correctly rounded quotient (and nbp_sid_to_float's IEEE division), in each channel and frame."""
    rng = np.random.default_rng(65535)
    host = [np.stack([rng.permutation(65536) for _ in range(3)], -1).astype(np.uint16).reshape(256, 256, 3)
            for _ in range(2)]
    device = [torch.from_numpy(a.view(np.int16)).to(dev) for a in host]
    ptrs = torch.tensor([t.data_ptr() for t in device], dtype=torch.int64).to(dev)
    hw = torch.tensor([[256, 256]] * 2, dtype=torch.int32).to(dev)
    _check((host, device, ptrs, hw), dev, [(0, 1, 0, 0), (1, 0, 0, 0)], [1.0, 300.0], 256, 256)


def test_bad_descriptor_raises_and_launches_nothing(monkeypatch):
    from lowlight_image_enhancement_amd.data import SonySIDResidentDataset, sony_sid_resident_dataset as mod
    ds = SonySIDResidentDataset(gold_opt(resident=BUDGET))
    good = ds[0]["desc"].tolist()
    ds.crop_batch(torch.tensor([good]), torch.ones(1))  # builds
    launched = []
    monkeypatch.setattr(mod, "call", lambda *a: launched.append(a))
    for bad in ([0, 2, 0, 0, 24, 24], [-1, 1, 0, 0, 24, 24], [0, 1, 41, 0, 24, 24], [0, 1, 0, 41, 24, 24],
                [0, 1, -1, 0, 24, 24], [0, 1, 0, 0, 65, 64]):
        with pytest.raises(ValueError):
            ds.crop_batch(torch.tensor([bad], dtype=torch.int32), torch.ones(1))
    with pytest.raises(ValueError):  # two window sizes in one batch
        ds.crop_batch(torch.tensor([good, [0, 1, 0, 0, 16, 16]], dtype=torch.int32), torch.ones(2))
    with pytest.raises(ValueError):  # one ratio per sample
        ds.crop_batch(torch.tensor([good], dtype=torch.int32), torch.ones(2))
    assert launched == []


def _drain(pf):
    out = []
    while True:
        batch = pf.next()
        if batch is None:
            return out
        out.append(batch)


KEYS = ("lq", "gt", "short", "long", "short_raw", "long_raw", "short_obs", "expo_ratio", "pair_id", "lq_path",
        "gt_path", "key")


def _assert_same_batches(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert set(a) == set(b)
        for k in KEYS:
            assert k in a, k
        assert a["short"] is a["lq"] and a["short_obs"] is a["lq"] and a["long"] is a["gt"] and a["long_raw"] is a["gt"]
        for k, v in b.items():
            if torch.is_tensor(v):
                assert a[k].is_cuda and a[k].dtype == v.dtype and torch.equal(a[k], v), k
            else:
                assert a[k] == v, k


def test_resident_dataset_end_to_end_train(dev):
    """SonySIDResidentDataset -> create_dataloader -> CUDAPrefetcher delivers, bit for bit, the batches of
    SonySIDLMDBDataset -> create_dataloader -> CUDAPrefetcher with the same options and seed, and the oracle's."""
    from lowlight_image_enhancement_amd.data import (CUDAPrefetcher, SonySIDLMDBDataset, SonySIDResidentDataset,
                                                     create_dataloader)
    opt = gold_opt(samples_per_pair=6)
    lopt = {"phase": "train", "batch_size_per_gpu": 2, "num_worker_per_gpu": 0, "pin_memory": True}
    base = SonySIDLMDBDataset(opt)
    want = _drain(CUDAPrefetcher(create_dataloader(base, lopt, sampler=torch.utils.data.SequentialSampler(base),
                                                   seed=0), {"num_gpu": 1}))
    ds = SonySIDResidentDataset(dict(opt, resident=BUDGET))
    loader = create_dataloader(ds, dict(lopt, num_worker_per_gpu=4), sampler=torch.utils.data.SequentialSampler(ds),
                               seed=0)
    assert loader.num_workers == 0 and ds._resident is None
    pf = CUDAPrefetcher(loader, {"num_gpu": 1})
    got = _drain(pf)
    assert len(got) == 3 and len(ds._resident.frames) == 2
    _assert_same_batches(got, want)
    s_full = osid.png_decode(read_gold("short/debugpair1_00_0.1s.png"))
    l_full = osid.png_decode(read_gold("long/debugpair1_00_1s.png"))
    rng = np.random.default_rng(123)
    for batch in got:
        assert batch["lq"].shape == (2, 3, 24, 24) and batch["expo_ratio"].shape == (2, 1, 1, 1)
        assert "desc" not in batch and batch["pair_id"] == ["debugpair1_00"] * 2
        for b in range(2):
            ref = osid.getitem_arrays(s_full, l_full, 10.0, osid.crop_window(rng, 64, 64, 24, "train", True))
            for k in ("lq", "gt", "short_raw", "long_raw"):
                assert np.array_equal(batch[k][b].cpu().numpy(), ref[k]), k
    pf.reset()  # a second epoch draws on, like the uint16 path
    again = _drain(pf)
    assert len(again) == 3 and not all(torch.equal(a["lq"], b["lq"]) for a, b in zip(again, got))


def test_resident_dataset_end_to_end_val(dev):
    """The val subset (disk backend) delivers the whole 64 x 64 frame."""
    from lowlight_image_enhancement_amd.data import (CUDAPrefetcher, SonySIDLMDBDataset, SonySIDResidentDataset,
                                                     create_dataloader)
    opt = gold_opt(phase="val", subset="val_small", samples_per_pair=1, io_backend=gold_disk_backend())
    want = _drain(CUDAPrefetcher(create_dataloader(SonySIDLMDBDataset(opt), {"phase": "val"}), {"num_gpu": 1}))
    got = _drain(CUDAPrefetcher(create_dataloader(SonySIDResidentDataset(dict(opt, resident=BUDGET)),
                                                  {"phase": "val"}), {"num_gpu": 1}))
    assert len(got) == 1 and got[0]["lq"].shape == (1, 3, 64, 64)
    _assert_same_batches(got, want)
    ref = osid.getitem_arrays(osid.png_decode(read_gold("short/debugpair2_00_0.1s.png")),
                              osid.png_decode(read_gold("long/debugpair2_00_1s.png")), 10.0, (0, 0, 64, 64))
    for k in ("lq", "gt", "short_raw", "long_raw"):
        assert np.array_equal(got[0][k][0].cpu().numpy(), ref[k]), k


def test_crop_batch_writes_into_caller_buffers(dev):
    from lowlight_image_enhancement_amd.data import SonySIDResidentDataset
    ds = SonySIDResidentDataset(gold_opt(resident=BUDGET))
    desc = torch.stack([ds[i]["desc"] for i in range(4)])
    ratio = torch.tensor([10.0, 100.0, 250.0, 0.5])
    want = ds.crop_batch(desc, ratio)
    bufs = tuple(torch.full((4, 3, 24, 24), -7.0, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = ds.crop_batch(desc, ratio.reshape(4, 1, 1, 1), out=bufs)
    torch.cuda.synchronize()
    # only the descriptors and the ratios went to the device: far less than one output (27 648 B)
    assert torch.cuda.max_memory_allocated() - before < bufs[0].numel() * 4 // 4
    assert all(g is b for g, b in zip(got, bufs))
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    for bad in (bufs[:2], (bufs[0], bufs[1], bufs[2][:2]), (bufs[0], bufs[1], bufs[2].cpu()),
                (bufs[0], bufs[1], bufs[2].double())):
        with pytest.raises(ValueError):
            ds.crop_batch(desc, ratio, out=bad)


def test_shared_long_frame_is_resident_once(tmp_path, dev):
    """Three short exposures share one long frame: 4 + 2 device allocations, each holding its PNG's pixels, and the
    batch cut from them (frames of six sizes, short and long of different widths) equals the oracle's."""
    from lowlight_image_enhancement_amd.data import SonySIDResidentDataset
    opt, arrays = write_shared_long_set(str(tmp_path), resident=dict(BUDGET, decode_threads=3))
    ds = SonySIDResidentDataset(opt)
    res = ds.build()
    assert res is ds.build()
    assert len(res.frames) == len(ds.plan.frames) == 6
    assert len({t.data_ptr() for t in res.frames}) == 6
    assert res.ptrs.tolist() == [t.data_ptr() for t in res.frames]
    assert res.hw.tolist() == [list(s) for s in ds.plan.shapes]
    for key, t in zip(ds.plan.frames, res.frames):
        assert t.dtype == torch.int16 and np.array_equal(t.cpu().numpy().view(np.uint16), arrays[key]), key
    samples = [ds[i] for i in range(len(ds))]
    desc = torch.stack([s["desc"] for s in samples])
    ratio = torch.stack([s["expo_ratio"] for s in samples])
    lq, sraw, gt = (t.cpu().numpy() for t in ds.crop_batch(desc, ratio))
    for b, s in enumerate(samples):
        ref = osid.getitem_arrays(arrays[("short", s["lq_path"])], arrays[("long", s["gt_path"])],
                                  float(s["expo_ratio"]), tuple(s["desc"].tolist()[2:]))
        assert np.array_equal(lq[b], ref["lq"]) and np.array_equal(sraw[b], ref["short_raw"])
        assert np.array_equal(gt[b], ref["gt"])
