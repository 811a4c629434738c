"""precision = "auto" without a GPU: the selection table (pick_precision), the new default and what it leaves alone
(state_dict, NAFNetLocal.from_net, the width check of the explicit 16-bit settings), and resolved_precision() on a
machine where torch.autocast("cuda") disables itself."""
import warnings

import pytest
import torch

W8 = dict(img_channel=3, width=8, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])
F16, BF16 = torch.float16, torch.bfloat16


@pytest.mark.parametrize("setting", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("on,adt", [(False, F16), (True, F16), (True, BF16), (False, BF16)])
@pytest.mark.parametrize("width", [32, 20])
def test_explicit_setting_ignores_autocast(setting, on, adt, width):
    from lowlight_image_enhancement_amd.nafnet import pick_precision
    assert pick_precision(setting, on, adt, width) == (setting, False)


@pytest.mark.parametrize("on,adt,width,expect", [
    (False, F16, 32, ("fp32", False)),   # no region, or autocast(enabled=False): the dtype is not looked at
    (False, BF16, 32, ("fp32", False)),
    (False, F16, 20, ("fp32", False)),   # nothing to warn about outside a region
    (True, F16, 32, ("fp16", False)),
    (True, BF16, 32, ("bf16", False)),
    (True, F16, 8, ("fp16", False)),
    (True, F16, 20, ("fp32", True)),     # width % 8: fp32 kernels, with the warning flag
    (True, BF16, 20, ("fp32", True)),
    (True, BF16, 12, ("fp32", True)),
])
def test_auto_follows_the_region(on, adt, width, expect):
    from lowlight_image_enhancement_amd.nafnet import pick_precision
    assert pick_precision("auto", on, adt, width) == expect


def test_unknown_setting_or_dtype_raises():
    from lowlight_image_enhancement_amd.nafnet import pick_precision
    with pytest.raises(ValueError):
        pick_precision("fp8", False, F16, 32)
    with pytest.raises(ValueError):
        pick_precision("auto", True, torch.float64, 32)


def test_default_is_auto_everywhere():
    from lowlight_image_enhancement_amd.nafnet import NAFNet, NAFNetLocal
    from lowlight_image_enhancement_amd.NewBP_model.newbp_net_arch import NewBPNAFNet, create_newbp_net
    net = NAFNet(**W8)
    assert net.precision == "auto"
    assert NAFNetLocal(**W8, train_size=(1, 3, 16, 16)).precision == "auto"
    assert NAFNetLocal.from_net(net, train_size=(1, 3, 16, 16)).precision == "auto"
    assert create_newbp_net(in_channels=3, width=8, enc_blk_nums=[1], middle_blk_num=1,
                            dec_blk_nums=[1]).precision == "auto"
    assert NewBPNAFNet(in_channels=3, width=8, enc_blk_nums=[1], middle_blk_num=1, dec_blk_nums=[1]).precision == "auto"


def test_from_net_follows_the_setting_and_pins_nothing():
    from lowlight_image_enhancement_amd.nafnet import NAFNet, NAFNetLocal
    net = NAFNet(**W8)
    net._active = "fp16"  # as if the view were made while the executor runs: the pin is not inherited
    view = NAFNetLocal.from_net(net, train_size=(1, 3, 16, 16))
    assert view.precision == "auto" and view._active is None
    net._active = None
    assert view.resolved_precision() == "fp32" and view.adt == torch.float32 and view.dt == 0


def test_state_dict_unaffected_by_the_setting():
    from lowlight_image_enhancement_amd.nafnet import NAFNet
    torch.manual_seed(0)
    net = NAFNet(**W8)
    base = {k: v.clone() for k, v in net.state_dict().items()}
    for setting in ("auto", "fp32", "fp16", "bf16"):
        net.precision = setting
        sd = net.state_dict()
        assert list(sd) == list(base)
        assert not any("precision" in k or "_active" in k for k in sd)
        for k in base:
            assert sd[k].dtype == torch.float32 and torch.equal(sd[k], base[k]), (setting, k)
    other = NAFNet(**W8)
    other.precision = "fp16"
    other.load_state_dict(base)
    assert other.precision == "fp16" and torch.equal(other.flat, net.flat)


def test_explicit_16bit_on_width_20_still_raises():
    from lowlight_image_enhancement_amd.nafnet import NAFNet
    net = NAFNet(img_channel=3, width=20, enc_blk_nums=[1], middle_blk_num=1, dec_blk_nums=[1])
    assert net.dt == 0  # "auto", no region
    for setting in ("fp16", "bf16"):
        net.precision = setting
        assert net.resolved_precision() == setting
        with pytest.raises(ValueError, match="multiple of 8"):
            net.dt
    net.precision = "fp32"
    assert net.dt == 0


def test_resolved_precision_where_the_region_disables_itself():
    """Without a GPU torch.autocast("cuda") warns and disables itself: "auto" resolves to fp32 inside it (with one,
    the region is live and selects its dtype)."""
    from lowlight_image_enhancement_amd.nafnet import NAFNet
    net = NAFNet(**W8)
    live = torch.cuda.is_available()
    assert net.resolved_precision() == "fp32"
    for adt, name, code in ((F16, "fp16", 2), (BF16, "bf16", 1)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with torch.autocast("cuda", dtype=adt):
                assert net.resolved_precision() == (name if live else "fp32")
                assert net.adt == (adt if live else torch.float32) and net.dt == (code if live else 0)
            with torch.autocast("cuda", dtype=adt, enabled=False):
                assert net.resolved_precision() == "fp32"
    net.precision = "bf16"
    assert net.resolved_precision() == "bf16" and net.adt == torch.bfloat16 and net.dt == 1


def test_the_pin_wins_over_setting_and_region_and_is_restored():
    from lowlight_image_enhancement_amd.nafnet import NAFNet, Tape
    net = NAFNet(**W8)
    with net._pinned("fp16"):
        assert net.adt == torch.float16 and net.dt == 2 and net.active_precision == "fp16"
        with net._pinned("fp32"):  # another tape's backward inside: restored on the way out
            assert net.adt == torch.float32 and net.dt == 0
        assert net.dt == 2
        assert net.precision == "auto"  # the setting itself is never written
    assert net._active is None and net.dt == 0
    with pytest.raises(RuntimeError):
        with net._pinned("bf16"):
            raise RuntimeError("an error inside the executor")
    assert net._active is None
    with pytest.raises(ValueError):
        with net._pinned("auto"):
            pass
    assert Tape("bf16").precision == "bf16" and Tape("fp32") == []
