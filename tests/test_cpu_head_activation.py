"""The `activation` argument of Unet on the host side: names and refusals, the module tree, the handle's setting and the
argument checks of the two single operators (nothing here enqueues a kernel)."""
import ctypes as C

import pytest
import torch

NAMES = [None, "identity", "sigmoid", "tanh", "softmax2d", "softmax", "logsoftmax", "clamp"]


def _unet(activation, **kw):
    from denoising_diffusion_deep_fake_amd import Unet
    return Unet("resnet18", None, 3, 3, activation, **kw)


@pytest.mark.parametrize("name", NAMES, ids=str)
def test_every_accepted_name_constructs(name):
    net = _unet(name)
    canonical = {"identity": None, "softmax": "softmax2d"}.get(name, name)
    assert net.activation == canonical
    head = net.segmentation_head
    assert len(head) == 3 and isinstance(head[0], torch.nn.Conv2d)
    if canonical is None:
        assert isinstance(head[2], torch.nn.Identity)
    else:
        assert canonical in repr(head[2]) and not list(head[2].parameters()) and not list(head[2].buffers())


def test_aliases_normalise_to_one_value():
    assert _unet("identity").activation is _unet(None).activation is None
    assert _unet("softmax").activation == _unet("softmax2d").activation == "softmax2d"


def test_refusals_say_why():
    for name in ("argmax", "argmax2d"):
        with pytest.raises(ValueError, match="integer tensor.*no gradient"):
            _unet(name)
    for fn in (torch.tanh, torch.nn.Tanh(), lambda t: t):
        with pytest.raises(ValueError, match="no device kernel for a Python callable"):
            _unet(fn)
    with pytest.raises(ValueError) as e:
        _unet("relu")
    assert str(e.value) == "Activation should be callable/sigmoid/softmax/logsoftmax/tanh/argmax/argmax2d/clamp/None; got relu"
    with pytest.raises(ValueError, match="Activation should be callable/sigmoid"):
        _unet(3)


def test_state_dict_and_parameter_count_are_those_of_a_plain_head():
    from denoising_diffusion_deep_fake_amd import Unet
    plain = Unet("resnet34", None, 3, 3, None)
    for name in ("tanh", "softmax2d", "clamp"):
        net = Unet("resnet34", None, 3, 3, name)
        assert list(net.state_dict().keys()) == list(plain.state_dict().keys())
        assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in plain.parameters()) == 24436659
        assert [n for n, _ in net.named_parameters()] == [n for n, _ in plain.named_parameters()]


def test_handle_setting_round_trips_on_either_kind_of_handle():
    from denoising_diffusion_deep_fake_amd import _lib
    L = _lib.lib()
    assert [_lib.ACT_IDENTITY, _lib.ACT_SIGMOID, _lib.ACT_TANH, _lib.ACT_SOFTMAX, _lib.ACT_LOGSOFTMAX, _lib.ACT_CLAMP] == \
        list(range(6))
    for nets in (1, 2):
        h = C.c_void_p()
        _lib.check(L.d3f_unet_create_nets(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, nets, nets, C.byref(h)))
        try:
            fwd0, dg0, wg0 = ((C.c_int32 * 16)() for _ in range(3))
            _lib.check(L.d3f_unet_plan_counts(h, fwd0, dg0, wg0))
            ws0 = L.d3f_unet_workspace_bytes(h)
            assert L.d3f_unet_head_activation(h) == _lib.ACT_IDENTITY
            for code in (_lib.ACT_TANH, _lib.ACT_CLAMP, _lib.ACT_SOFTMAX, _lib.ACT_IDENTITY, _lib.ACT_SIGMOID, _lib.ACT_LOGSOFTMAX):
                assert L.d3f_unet_set_head_activation(h, code) == 0
                assert L.d3f_unet_head_activation(h) == code
            for bad in (-1, 6, 100):
                assert L.d3f_unet_set_head_activation(h, bad) != 0
                assert b"unknown code" in L.d3f_last_error()
                assert L.d3f_unet_head_activation(h) == _lib.ACT_LOGSOFTMAX  # unchanged by a refused call
            # the setting is no part of the plan: same kernels, same workspace (a buffer sized before the call still fits)
            fwd1, dg1, wg1 = ((C.c_int32 * 16)() for _ in range(3))
            _lib.check(L.d3f_unet_plan_counts(h, fwd1, dg1, wg1))
            assert (list(fwd0), list(dg0), list(wg0)) == (list(fwd1), list(dg1), list(wg1))
            assert L.d3f_unet_workspace_bytes(h) == ws0
        finally:
            L.d3f_unet_destroy(h)
    assert L.d3f_unet_head_activation(None) < 0 and L.d3f_unet_set_head_activation(None, 0) != 0


def test_single_operators_refuse_bad_arguments_before_anything_is_enqueued():
    """C = 0, C = 17, Cpad < C and an unknown code: D3F_EINVAL from the host-side check -- the pointers are null, so a
    call that got as far as a launch would not return an argument error"""
    from denoising_diffusion_deep_fake_amd import _lib
    L = _lib.lib()
    for act, Cc, msg in ((_lib.ACT_TANH, 0, b"0 channels"), (_lib.ACT_TANH, 17, b"17 channels"), (6, 3, b"unknown code"),
                         (-1, 3, b"unknown code")):
        assert L.d3f_head_activation_forward(act, None, None, 2, Cc, 6, 10, None) == -1
        assert msg in L.d3f_last_error()
        for dtype in (_lib.F32, _lib.BF16):
            assert L.d3f_head_activation_backward(act, dtype, None, None, None, None, 2, Cc, 6, 10, 24, None) == -1
            assert msg in L.d3f_last_error()
    assert L.d3f_head_activation_backward(_lib.ACT_SIGMOID, _lib.F32, None, None, None, None, 2, 5, 6, 10, 4, None) == -1
    assert b"padded channels 4 < channels 5" in L.d3f_last_error()


def test_ops_resolve_names_and_codes():
    from denoising_diffusion_deep_fake_amd import _lib, ops
    assert ops.head_activation_code("softmax") == ops.head_activation_code("softmax2d") == _lib.ACT_SOFTMAX
    assert ops.head_activation_code(None) == ops.head_activation_code("identity") == _lib.ACT_IDENTITY
    assert ops.head_activation_code(_lib.ACT_CLAMP) == _lib.ACT_CLAMP
    with pytest.raises(ValueError):
        ops.head_activation_code("argmax")
    with pytest.raises(_lib.D3FError):  # no CPU fallback
        ops.head_activation_forward("tanh", torch.zeros(1, 3, 4, 4))


def test_pair_of_differently_activated_networks_is_refused():
    from denoising_diffusion_deep_fake_amd import UnetPair
    with pytest.raises(ValueError, match="differ in activation"):
        UnetPair(_unet("tanh"), _unet(None))
    UnetPair(_unet("tanh"), _unet("tanh"))


def test_trainers_read_the_optional_hparam():
    from denoising_diffusion_deep_fake_amd.balance_training_images.lit_module import LitModule as Balance
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule as Fake
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule as Denoiser
    common = dict(batch_size=2, learning_rate=0.01, max_epochs=1, cosine_scheduler_max_epoch=2, num_workers=0,
                  encoder_name="resnet18", noise_exponential_sampling_lambda=5, synthetic=True, image_size=64)
    den = dict(common, mean=[128] * 3, std=[128] * 3)
    assert Denoiser(**den).model.activation is None and "activation" not in Denoiser(**den).hparams
    lit = Denoiser(**den, activation="tanh")
    assert lit.model.activation == "tanh" and lit.hparams["activation"] == "tanh"
    fake = Fake(**dict(common, mode="denoise", adam_b1=0.5, adam_b2=0.999, mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3,
                       std_b=[0.5] * 3, ema_beta=0.9999, ema_update_every=1), activation="sigmoid")
    assert fake.model_a.activation == fake.model_b.activation == "sigmoid"
    assert Balance(**den, ratio_of_noise=0.2, number_of_classes=4, activation="clamp").model.activation == "clamp"
