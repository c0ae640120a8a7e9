"""The `activation` argument of Unet on the device.

The operator (csrc/head_act.hip) is checked against float64 on its own (test 1).  Everything else reduces an activated
network, bit for bit, to the identity-head network -- which the existing suites pin to the oracle -- composed with that
operator: forward in train / eval / graph mode, backward, the pair engine, the fused uint8 entries and one training
step."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = ["identity", "sigmoid", "tanh", "softmax2d", "logsoftmax", "clamp"]
NET_ACTS = ["tanh", "sigmoid", "softmax2d", "clamp"]

_TORCH = {
    "identity": lambda z: z * 1,
    "sigmoid": torch.sigmoid,
    "tanh": torch.tanh,
    "softmax2d": lambda z: torch.softmax(z, dim=1),
    "logsoftmax": lambda z: torch.log_softmax(z, dim=1),
    "clamp": lambda z: torch.clamp(z, 0, 1),
}


@functools.lru_cache(maxsize=None)
def _operator_case(act, Cc):
    """inputs (fp32) and the two yardsticks of one operator case, computed once: the float64 result and e_ref, the
    max-abs distance of torch's CPU fp32 result from it, forward and backward"""
    gen = torch.Generator().manual_seed(1000 + 17 * Cc + ACTS.index(act))
    z = 3 * torch.randn((2, Cc, 6, 10), generator=gen)
    z.view(-1)[::7] *= 10  # saturating values near +-90: an unstabilised softmax or sigmoid overflows there
    g = torch.randn(z.shape, generator=gen)
    res = {}
    for dt in (torch.float64, torch.float32):
        zz = z.to(dt).requires_grad_(True)
        a = _TORCH[act](zz)
        a.backward(g.to(dt))
        res[dt] = (a.detach(), zz.grad.detach())
    a64, dz64 = res[torch.float64]
    e_fwd = (res[torch.float32][0].double() - a64).abs().max().item()
    e_bwd = (res[torch.float32][1].double() - dz64).abs().max().item()
    return z, g, a64, dz64, e_fwd, e_bwd


def _within(got, want64, e_ref, what):
    err = (got.double().cpu() - want64).abs().max().item()
    print(f"{what}: max-abs error {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref if e_ref else float('nan'):.2f}")
    assert torch.isfinite(got).all(), what
    if e_ref == 0:
        assert torch.equal(got.double().cpu(), want64), (what, err)
    else:
        assert err <= 8 * e_ref, (what, err, e_ref)


@pytest.mark.parametrize("Cc", [1, 3, 16])
@pytest.mark.parametrize("act", ACTS)
def test_operator_against_float64(act, Cc):
    """Forward and backward within 8 x e_ref of float64 in max-abs, e_ref = torch's CPU fp32 distance from float64 on the
    same inputs (the device expf / tanhf / logf are specified to 1-2 ulp where the host's are <= 1, and an activation
    chains up to three of them plus a divide); exact where e_ref is 0.  HW = 60 is no multiple of the block or of 4."""
    from denoising_diffusion_deep_fake_amd import ops
    z, g, a64, dz64, e_fwd, e_bwd = _operator_case(act, Cc)
    zc, gc = z.cuda(), g.cuda()
    a = ops.head_activation_forward(act, zc)
    _within(a, a64, e_fwd, f"{act} C={Cc} forward")
    for cpad in sorted({(Cc + 3) // 4 * 4, (Cc + 7) // 8 * 8, (Cc + 7) // 8 * 8 + 8 * (Cc == 16)}):
        dz, dy = ops.head_activation_backward(act, zc, gc, ops.F32, cpad)
        _within(dz, dz64, e_bwd, f"{act} C={Cc} Cpad={cpad} backward")
        assert dy.shape == (2, 6, 10, cpad) and dy.dtype == torch.float32
        assert torch.equal(dy[..., :Cc].view(torch.int32), dz.permute(0, 2, 3, 1).contiguous().view(torch.int32))
        assert torch.equal(dy[..., Cc:].view(torch.int32), torch.zeros_like(dy[..., Cc:]).view(torch.int32))
        dzb, dyb = ops.head_activation_backward(act, zc, gc, ops.BF16, cpad)
        assert torch.equal(dzb, dz) and dyb.dtype == torch.bfloat16
        assert torch.equal(dyb[..., :Cc].view(torch.int16), dz.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous().view(torch.int16))
        assert torch.equal(dyb[..., Cc:].view(torch.int16), torch.zeros_like(dyb[..., Cc:]).view(torch.int16))


def _net(activation, dtype, encoder="resnet18", classes=3, seed=3):
    from denoising_diffusion_deep_fake_amd import Unet
    torch.manual_seed(seed)
    net = Unet(encoder, None, 3, classes, activation, compute_dtype=dtype)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
        net.segmentation_head[0].bias.normal_(0, 0.1)
    return net.cuda().train()


def _pair_of_nets(act, dtype, **kw):
    """network N with a plain head and network A with the activation, same parameters and statistics"""
    n = _net(None, dtype, **kw)
    a = _net(act, dtype, **kw)
    a.load_state_dict(n.state_dict())
    return n, a.cuda().train()


def _x(B=2, S=64, seed=11):
    from denoising_diffusion_deep_fake_amd.dataset import synthetic_face_crops
    return synthetic_face_crops(B, (S, S), seed=seed, device="cuda")


def _clear_grads(*nets):
    for net in nets:
        for p in net.parameters():
            p.grad = None


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_identity_is_todays_network(dtype):
    x, g = _x(), torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    nets = [_net(act, dtype, encoder="resnet34") for act in (None, "identity")]
    outs = []
    for net in nets:
        pred = net(x)
        pred.backward(g)
        outs.append((pred.detach(), net.flat_grads))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[0][1]).all() and outs[0][1].abs().max() > 0


def _forward_composition(act, dtype, classes):
    from denoising_diffusion_deep_fake_amd import ops
    n, a = _pair_of_nets(act, dtype, classes=classes)
    x = _x()
    with torch.no_grad():
        for step in range(2):  # train mode, twice: the second pass starts from the running statistics of the first
            want = ops.head_activation_forward(act, n(x))
            got = a(x)
            assert torch.equal(got, want), (act, dtype, "train", step)
            assert torch.equal(a.flat_bn_stats, n.flat_bn_stats)
            assert int(a.encoder.bn1.num_batches_tracked) == int(n.encoder.bn1.num_batches_tracked) == step + 1
        n.eval(), a.eval()
        z = n(x)
        want = ops.head_activation_forward(act, z)
        assert torch.equal(a(x), want), (act, dtype, "eval")
        xb = x.clone()
        for it in range(2):  # capture, then replay
            assert torch.equal(a.forward_graph(xb), want), (act, dtype, "graph", it)
        assert not torch.equal(want, z)  # the head is active


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("act", NET_ACTS)
def test_forward_composition_is_bitwise(act, dtype):
    """A(x) == activation operator(N(x)) in train, eval and graph mode, equal running statistics: with the operator
    checked against float64 above and the identity network pinned to the oracle by the existing suites, no float64
    network pass is needed here"""
    _forward_composition(act, dtype, 3)


def test_forward_composition_with_sixteen_classes():
    _forward_composition("softmax2d", "f32", 16)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("act", NET_ACTS)
def test_backward_composition_is_bitwise(act, dtype):
    """A's gradient for upstream g == N's gradient for dz = operator backward(z = N(x), g): every parameter
    (24 436 659 values), the head's bias included.  A's returned prediction is overwritten with NaN before backward: the engine reads its own z."""
    from denoising_diffusion_deep_fake_amd import _lib, ops
    n, a = _pair_of_nets(act, dtype, encoder="resnet34")
    x, g = _x(), torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    z = n(x)
    dz = ops.head_activation_backward(act, z.detach(), g)[0]
    z.backward(dz)
    pred = a(x)
    pred.detach().fill_(float("nan"))
    pred.backward(g)
    # every parameter of the resnet34 network: the engine's table, the module tree and the flat gradient agree
    params = list(a.parameters())
    assert len(params) == len(a._table()[0]) == len(list(n.parameters()))
    assert sum(p.numel() for p in params) == a.flat_grads.numel() == 24436659
    assert all(p.grad is not None for p in params)
    assert torch.isfinite(a.flat_grads).all()
    assert torch.equal(a.flat_grads, n.flat_grads), (act, dtype)
    bias = a.segmentation_head[0].bias.grad
    assert torch.equal(bias, n.segmentation_head[0].bias.grad) and bias.abs().max() > 0
    if act == "tanh":  # the gradient-bucket route: d3f_unet_backward_nojoin bucket by bucket, then the join
        one_call = a.flat_grads.clone()
        _clear_grads(a)
        a.flat_grads.zero_()
        calls = []
        a.set_grad_sync(lambda k, sl: calls.append(k), 4)
        a(x).backward(g)
        a.set_grad_sync(None)
        assert calls == [0, 1, 2, 3]
        assert torch.equal(a.flat_grads, one_call)
        # the head of that pass turned z into dz in place: a second pass over the same forward is refused, not wrong
        eng, scratch = a._rt["last_engine"], torch.empty_like(a.flat_grads)
        rc = _lib.lib().d3f_unet_backward(eng.h, _lib.ptr(a.flat_params), _lib.ptr(g), _lib.ptr(scratch),
                                          _lib.ptr(eng.workspace), 0, eng.nseg, _lib.stream_ptr())
        assert rc != 0 and b"one backward pass per training forward" in _lib.lib().d3f_last_error()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pair_of_tanh_networks_is_bitwise_each_network_alone(dtype):
    from denoising_diffusion_deep_fake_amd import UnetPair
    nets = [_net("tanh", dtype, encoder="resnet34", seed=3 + i) for i in range(2)]
    twins = [copy.deepcopy(n).cuda().train().set_plan_nets(2) for n in nets]
    assert all(t.activation == "tanh" for t in twins)
    xs = [_x(seed=30 + i) for i in range(2)]
    gs = [torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(50 + i)).cuda() for i in range(2)]
    pair = UnetPair(*nets)
    for step in range(2):
        _clear_grads(*nets, *twins)
        preds = pair(*xs)
        kept = [p.detach().clone() for p in preds]
        torch.autograd.backward(list(preds), gs)
        for i in range(2):
            alone = twins[i](xs[i])
            alone.backward(gs[i])
            assert torch.equal(kept[i], alone.detach()), (step, i, "prediction")
            assert kept[i].abs().max() <= 1
            assert torch.equal(nets[i].flat_grads, twins[i].flat_grads), (step, i, "gradient")
            assert torch.equal(nets[i].flat_bn_stats, twins[i].flat_bn_stats), (step, i, "running statistics")
    assert not torch.equal(kept[0], kept[1]) and not torch.equal(nets[0].flat_grads, nets[1].flat_grads)


def test_uint8_entries_apply_the_activation():
    """predict_u8 eager and graph-replayed and the right half of predict_frames_u8 give the bytes of the unfused route
    (cv2_to_tensor_normalised -> eval forward -> tensor_cv2_to_denormalised); a tanh and a plain head over the same
    buffers differ, each equal to its own unfused route; a changed setting drops the captured graph"""
    from denoising_diffusion_deep_fake_amd import _lib
    from denoising_diffusion_deep_fake_amd.train_deep_fake.lit_module import LitModule
    hp = dict(mode="denoise", batch_size=2, learning_rate=0.01, adam_b1=0.5, adam_b2=0.999, max_epochs=1,
              cosine_scheduler_max_epoch=50, num_workers=0, encoder_name="resnet18", noise_exponential_sampling_lambda=3,
              mean_a=[0.5] * 3, std_a=[0.5] * 3, mean_b=[0.5] * 3, std_b=[0.5] * 3, synthetic=True, image_size=64,
              synthetic_length=4, ema_beta=0.9999, ema_update_every=1, augment=False)
    torch.manual_seed(6)
    lits = {act: LitModule(**hp, activation=act).cuda().eval() for act in ("tanh", None)}
    nets = {act: lit.model_a for act, lit in lits.items()}
    assert nets["tanh"].activation == "tanh" and nets[None].activation is None
    with torch.no_grad():  # non-trivial running statistics, a head that leaves [-1, 1]
        for name, buf in nets["tanh"].named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0, 0.1)
            elif name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
        nets["tanh"].segmentation_head[0].weight.mul_(3)
    nets[None].load_state_dict(nets["tanh"].state_dict())
    mean, std = [0.4, 0.5, 0.6], [0.5, 0.45, 0.55]
    mt, st = torch.tensor(mean, device="cuda"), torch.tensor(std, device="cuda")
    frames = np.random.default_rng(1).integers(0, 256, size=(2, 64, 64, 3), dtype=np.uint8)
    buf_in = torch.from_numpy(frames).cuda()
    buf_out = torch.empty_like(buf_in)

    def unfused(act):
        lit, net = lits[act], nets[act]
        with torch.no_grad():
            y = net(torch.cat([lit.cv2_to_tensor_normalised(f, mt, st) for f in frames]))
            return np.stack([lit.tensor_cv2_to_denormalised(y[i:i + 1], mt, st) for i in range(2)])

    got = {}
    for act, net in nets.items():
        want = unfused(act)
        eager = net.predict_u8(buf_in, mean, std, graph=False).cpu().numpy()
        assert np.array_equal(eager, want), (act, np.abs(eager.astype(int) - want.astype(int)).max())
        for it in range(2):  # capture, then replay
            replay = net.predict_u8(buf_in, mean, std, graph=True, out=buf_out).cpu().numpy()
            assert np.array_equal(replay, want), (act, it)
        for graph in (False, True, True):
            pair = net.predict_frames_u8(buf_in, (64, 64), mean, std, graph=graph).cpu().numpy()
            assert np.array_equal(pair[:, :, :64], frames) and np.array_equal(pair[:, :, 64:], want), (act, graph)
        got[act] = want
    assert not np.array_equal(got["tanh"], got[None])
    # the setting changes on a live engine whose predict graph is captured for (buf_in, buf_out): the next replay must
    # run the new head
    eng = nets["tanh"]._rt["last_engine"]
    L = _lib.lib()
    assert L.d3f_unet_head_activation(eng.h) == _lib.ACT_TANH
    try:
        _lib.check(L.d3f_unet_set_head_activation(eng.h, _lib.ACT_IDENTITY))
        plain = nets["tanh"].predict_u8(buf_in, mean, std, graph=True, out=buf_out).cpu().numpy()
        assert np.array_equal(plain, got[None])
    finally:
        _lib.check(L.d3f_unet_set_head_activation(eng.h, _lib.ACT_TANH))
    again = nets["tanh"].predict_u8(buf_in, mean, std, graph=True, out=buf_out).cpu().numpy()
    assert np.array_equal(again, got["tanh"])


def test_one_training_step_with_a_tanh_head(tmp_path):
    from denoising_diffusion_deep_fake_amd.train_denoiser.lit_module import LitModule
    from denoising_diffusion_deep_fake_amd.trainer import Trainer
    hp = dict(batch_size=4, learning_rate=0.02, max_epochs=1, cosine_scheduler_max_epoch=2, num_workers=0,
              encoder_name="resnet34", noise_exponential_sampling_lambda=5, mean=[128, 128, 128], std=[128, 128, 128],
              synthetic=True, image_size=64, augment=False, synthetic_length=8)
    x = _x(B=4, seed=21)
    preds = {}
    for act in ("tanh", None):
        torch.manual_seed(5)
        lit = LitModule(**dict(hp, activation=act)) if act else LitModule(**hp)
        before = copy.deepcopy(lit.model.state_dict())
        tr = Trainer(max_epochs=1, max_steps=1, default_root_dir=tmp_path / str(act), enable_checkpointing=False).fit(lit)
        assert tr.global_step == 1
        assert torch.isfinite(torch.as_tensor(lit._logged["loss"])).all()
        moved = max((v.cpu().float() - before[k].float()).abs().max().item() for k, v in lit.model.state_dict().items()
                    if k.endswith("weight"))
        assert moved > 0.01  # Adam's first step moves every element by ~lr
        lit.train()
        with torch.no_grad():
            preds[act] = lit.model(x)
        if act:
            tr.save_checkpoint(tmp_path / "tanh.ckpt")
            trained = lit
    assert torch.isfinite(preds["tanh"]).all() and preds["tanh"].abs().max() <= 1
    assert preds[None].abs().max() > 1  # the plain head leaves the range: the activation is what keeps A inside
    ck = torch.load(tmp_path / "tanh.ckpt", map_location="cpu", weights_only=False)
    assert ck["hyper_parameters"]["activation"] == "tanh"
    again = LitModule.load_from_checkpoint(tmp_path / "tanh.ckpt").cuda().eval()
    assert again.model.activation == "tanh" and "tanh" in repr(again.model.segmentation_head)
    trained.eval()
    with torch.no_grad():
        want = trained.model(x)
        assert torch.equal(again.model(x), want) and want.abs().max() <= 1
