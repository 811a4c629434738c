"""Host side of the validation pass, no GPU: quantile_rank against torch.quantile's own arithmetic, the Validator's
option handling, and the idx % world_size sharding with the final all_reduce over gloo (2 ranks, a stub metric on CPU
tensors; no kernel is launched)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

# torch.quantile accepts at most 2^24 elements; (n, q) as listed with the feature
RANK_CASES = [(1, 0.85), (2, 0.5), (101, 0.85), (1517, 0.85), (70001, 0.85), (12121088, 0.85), (16777216, 0.85)]


@pytest.mark.parametrize("n,q", RANK_CASES)
def test_quantile_rank_reproduces_torch_quantile_on_arange(n, q):
    from lowlight_image_enhancement_amd.metrics.valstats import quantile_rank
    x = torch.arange(n, dtype=torch.float32)  # already sorted
    k_lo, k_hi, w = quantile_rank(n, q)
    assert 0 <= k_lo <= k_hi < n and 0.0 <= w < 1.0
    got = torch.lerp(x[k_lo], x[k_hi], w)
    ref = torch.quantile(x, q)
    assert got.view(torch.int32).item() == ref.view(torch.int32).item(), (n, q, k_lo, k_hi, w, got.item(), ref.item())


def test_quantile_rank_known_values_and_validation():
    from lowlight_image_enhancement_amd.metrics.valstats import quantile_rank
    assert quantile_rank(1517, 0.85) == (1288, 1289, 0.5999755859375)
    assert quantile_rank(12121088, 0.85) == (10302924, 10302924, 0.0)
    assert quantile_rank(101, 0.85) == (85, 85, 0.0)
    assert quantile_rank(2 ** 24 + 5, 1.0)[1] == 2 ** 24 + 4  # no cap at 2^24, ranks stay inside the row
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            quantile_rank(10, bad)
    with pytest.raises(ValueError):
        quantile_rank(0, 0.5)


def test_quantile_rank_random_row_bit_for_bit():
    from lowlight_image_enhancement_amd.metrics.valstats import quantile_rank
    x = torch.randn(1517, generator=torch.Generator().manual_seed(1517))
    s = torch.sort(x).values
    for q in (0.85, 0.95, 0.5):
        k_lo, k_hi, w = quantile_rank(1517, q)
        got, ref = torch.lerp(s[k_lo], s[k_hi], w), torch.quantile(x, q)
        assert got.view(torch.int32).item() == ref.view(torch.int32).item(), (q, got.item(), ref.item())


def test_validator_option_handling():
    from lowlight_image_enhancement_amd import Validator
    from lowlight_image_enhancement_amd.validation import SUPPORTED_METRICS
    with pytest.raises(ValueError) as e:
        Validator({"metrics": {"niqe": {"type": "calculate_niqe"}}}, device="cpu")
    for t in SUPPORTED_METRICS:
        assert t in str(e.value)
    assert len(SUPPORTED_METRICS) == 6
    for key in ("use_image", "save_img"):
        with pytest.raises(NotImplementedError):
            Validator({key: True, "metrics": {"psnr": {"type": "linear_psnr"}}}, device="cpu")
    # the reference configs' keyword arguments, and the keys val_forward reads
    v = Validator({"grids": True, "crop_size_h": 256, "crop_size_w": 256, "max_minibatch": 8, "use_image": False,
                   "metrics": {"psnr": {"type": "linear_psnr", "data_range": 1.0},
                               "ssim": {"type": "linear_ssim", "data_range": 1.0},
                               "lpips": {"type": "lpips_distance", "net": "vgg"},
                               "de": {"type": "deltae2000_mean", "whitepoint": "D65-2"},
                               "de95": {"type": "deltae2000_p95", "whitepoint": "D65-2"},
                               "edge": {"type": "edge_deltae2000_mean", "whitepoint": "D65-2", "q": 0.85}}},
                  device="cpu")
    assert v.names == ["psnr", "ssim", "lpips", "de", "de95", "edge"]
    assert v.result() == {}  # zero items: an empty dict
    with pytest.raises(ValueError):
        Validator({"metrics": {"edge": {"type": "edge_deltae2000_mean", "q": 1.0}}}, device="cpu")
    with pytest.raises(ValueError):
        Validator({"metrics": {"psnr": {"type": "linear_psnr", "data_range": 0.0}}}, device="cpu")


def _stub_mean(pred, gt, scale=1.0):
    return (pred.double().mean() + gt.double().mean()) * scale


def test_validator_run_accepts_both_key_pairs_and_restores_mode():
    from lowlight_image_enhancement_amd.validation import Validator, register_metric
    register_metric("stub_mean", _stub_mean)
    v = Validator({"metrics": {"m": {"type": "stub_mean", "scale": 0.5}}}, device="cpu")
    net = torch.nn.Identity()
    net.train()
    items = [{"lq": torch.full((1, 3, 4, 4), 1.0), "gt": torch.full((1, 3, 4, 4), 3.0)},
             {"short": torch.full((1, 3, 4, 4), 5.0), "long": torch.full((1, 3, 4, 4), 7.0)}]
    out = v.run(net, items)
    assert list(out) == ["m"] and out["m"] == pytest.approx((2.0 + 6.0) / 2)
    assert net.training
    net.eval()
    assert v.run(net, items[:1])["m"] == pytest.approx(2.0) and not net.training  # run() starts from zero
    v.update(items[0]["lq"], items[0]["gt"])
    assert v.result()["m"] == pytest.approx(2.0)
    v.reset()
    assert v.result() == {}
    assert v.run(net, []) == {}
    with pytest.raises(ValueError):
        v.run(net, [{"input": items[0]["lq"]}])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lowlight_image_enhancement_amd.validation import Validator, register_metric
        seen = []

        def stub(pred, gt):
            seen.append(int(pred.flatten()[0].item()))
            return pred.double().mean()

        register_metric("stub_item", stub)
        v = Validator({"metrics": {"item": {"type": "stub_item"}}}, device="cpu")
        items = [{"lq": torch.full((1, 3, 4, 4), float(i)), "gt": torch.zeros(1, 3, 4, 4)} for i in range(5)]
        out = v.run(torch.nn.Identity(), items)  # rank and world size from torch.distributed
        q.put((rank, seen, dict(out)))
    finally:
        dist.destroy_process_group()


def test_validator_shards_items_and_reduces_over_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == [0, 2, 4] and res[1][1] == [1, 3]
    for _, _, out in res:
        assert out == {"item": pytest.approx(2.0)}  # the mean over all 5 items on both ranks
