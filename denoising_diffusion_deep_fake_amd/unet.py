"""`Unet(encoder_name, encoder_weights, in_channels, classes, activation)` -- drop-in for the
`segmentation_models_pytorch.Unet` object the reference builds at
d3f/train_denoiser/lit_module.py:46-52 and d3f/train_deep_fake/lit_module.py:53-59.

What callers rely on and what this class keeps:
  * constructor signature and error behaviour (unknown encoder -> KeyError, H/W not divisible
    by 32 -> RuntimeError);
  * `__call__(Tensor[B,C,H,W] f32) -> Tensor[B,classes,H,W]`, autograd through it;
  * `.parameters()` are ordinary leaf `nn.Parameter`s (torch.optim.Adam works on them),
    `state_dict()` keys are smp's (`encoder.layer1.0.conv1.weight`, `decoder.blocks.0.conv1.0.weight`,
    `segmentation_head.0.bias`, BatchNorm buffers incl. `num_batches_tracked`);
  * `copy.deepcopy`, `.train()/.eval()/.cuda()/.to()` (EMA wrapper, video script).

How it runs: every parameter is a view into ONE flat f32 buffer (likewise gradients and BN
running statistics), and forward/backward are single calls into libd3f_hip.so's whole-network
engine (csrc/engine.hip), which enqueues the hand-written gfx950 kernels on the current
stream.  There is no eager / CPU fallback: tensors must live on a HIP device.
"""
import ctypes as C
import os

import torch
import torch.nn as nn

from . import _lib
from ._lib import D3FError, check, ptr, ptr2, stream_ptr

_DTYPES = {"f32": _lib.F32, "fp32": _lib.F32, "float32": _lib.F32, torch.float32: _lib.F32,
           "bf16": _lib.BF16, "bfloat16": _lib.BF16, torch.bfloat16: _lib.BF16,
           "f32x3": _lib.F32X3}


# ---------------------------------------------------------------------------------------------
# parameter containers: same module tree (hence the same state_dict keys and initialisation)
# as torchvision ResNet + smp UnetDecoder.  Their forward() is never used.
# ---------------------------------------------------------------------------------------------
class _BasicBlock(nn.Module):
    def __init__(self, inplanes, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False),
                                            nn.BatchNorm2d(planes))


class _Encoder(nn.Module):
    def __init__(self, in_channels, blocks):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for li, n in enumerate(blocks, start=1):
            planes = 64 << (li - 1)
            layers = []
            for bi in range(n):
                layers.append(_BasicBlock(inplanes, planes, 2 if (bi == 0 and li > 1) else 1))
                inplanes = planes
            setattr(self, f"layer{li}", nn.Sequential(*layers))
        for m in self.modules():  # torchvision ResNet init
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")


class _DecoderBlock(nn.Module):
    def __init__(self, cin, cskip, cout):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(cin + cskip, cout, 3, padding=1, bias=False),
                                   nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
        self.attention1 = nn.Identity()
        self.conv2 = nn.Sequential(nn.Conv2d(cout, cout, 3, padding=1, bias=False),
                                   nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
        self.attention2 = nn.Identity()


class _Decoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.center = nn.Identity()
        spec = [(512, 256, 256), (256, 128, 128), (128, 64, 64), (64, 64, 32), (32, 0, 16)]
        self.blocks = nn.ModuleList([_DecoderBlock(*s) for s in spec])
        for m in self.modules():  # smp initialize_decoder
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, mode="fan_in", nonlinearity="relu")


_ENCODERS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}

# names of smp's Activation module -> the canonical name `Unet.activation` holds (a key of _lib.HEAD_ACTIVATIONS)
_ACTIVATION_NAMES = {None: None, "identity": None, "sigmoid": "sigmoid", "tanh": "tanh", "softmax2d": "softmax2d",
                     "softmax": "softmax2d", "logsoftmax": "logsoftmax", "clamp": "clamp"}


def canonical_activation(activation):
    """the `activation` argument of smp.Unet -> None / "sigmoid" / "tanh" / "softmax2d" / "logsoftmax" / "clamp";
    ValueError for what the HIP path does not run"""
    if activation in ("argmax", "argmax2d"):
        raise ValueError(f"Activation {activation} returns an integer tensor and has no gradient: the HIP path trains "
                         "through its head and does not offer argmax heads")
    if callable(activation):
        raise ValueError(f"Activation {activation!r} is a Python callable: there is no device kernel for a Python "
                         "callable (use sigmoid/softmax/logsoftmax/tanh/clamp/None)")
    if not (activation is None or isinstance(activation, str)) or activation not in _ACTIVATION_NAMES:
        raise ValueError("Activation should be callable/sigmoid/softmax/logsoftmax/tanh/argmax/argmax2d/clamp/None; "
                         f"got {activation}")
    return _ACTIVATION_NAMES[activation]


class _HeadActivation(nn.Module):
    """Last child of `segmentation_head` for an activated head: parameter-free, shows the activation in repr.  Its
    forward() is never used: the engine applies the activation (csrc/head_act.hip)."""

    def __init__(self, name):
        super().__init__()
        self.name = name

    def extra_repr(self):
        return self.name


class _Engine:
    """one libd3f_hip whole-network plan + its workspace, for a fixed (B, H, W, dtype)."""

    def __init__(self, encoder_name, in_channels, classes, B, H, W, dtype, device, nets, plan_nets, activation=None):
        # nets = 2: a pair, B images PER network; plan_nets = 2 with nets = 1: one network planned like the pair
        L = _lib.lib()
        self.h = C.c_void_p()
        check(L.d3f_unet_create_nets(encoder_name.encode(), in_channels, classes, B, H, W, dtype, nets, plan_nets,
                                     C.byref(self.h)))
        if activation is not None:  # (a handle starts as identity)
            check(L.d3f_unet_set_head_activation(self.h, _lib.HEAD_ACTIVATIONS[activation]))
        self.nets = nets
        self.net_stride = L.d3f_unet_net_workspace_stride(self.h)
        self.shape = (B, H, W)
        self.dtype = dtype
        self.workspace = torch.empty(L.d3f_unet_workspace_bytes(self.h), dtype=torch.uint8, device=device)
        if os.environ.get("D3F_POISON_WORKSPACE"):  # test hook: any read-before-write shows up as NaN
            self.workspace.fill_(0xFF)
        self.packed_version = None
        self._bn_cb = None
        self._side = False    # not asked yet
        self.serial = 0       # bumped by every forward that overwrites this workspace
        self.in_use = False   # a recorded autograd graph still needs this workspace's activations
        self.fwd_flops = L.d3f_unet_forward_flops(self.h)
        self.bwd_flops = L.d3f_unet_backward_flops(self.h)
        self.nseg = L.d3f_unet_num_segments(self.h)
        self.seg_ranges = []
        for s in range(self.nseg):
            b, e = C.c_int64(), C.c_int64()
            check(L.d3f_unet_segment_range(self.h, s, C.byref(b), C.byref(e)))
            self.seg_ranges.append((b.value, e.value))

    def set_bn_sync(self, group, world_size):
        """install (group given) or remove (None) the BatchNorm statistics all-reduce of this plan: the C engine calls
        back with a pointer into this workspace, the callback sums it over the ranks of `group` on the current stream"""
        L = _lib.lib()
        if group is None:
            check(L.d3f_unet_set_bn_sync(self.h, None, None, 1))
            self._bn_cb = None
            return
        import torch.distributed as dist
        ws = self.workspace
        base = ws.data_ptr()
        dev = ws.device
        err = self._bn_err = [None]  # the closure holds the workspace / group / this list, never the engine itself

        def allreduce(ctx, data, count, stream):
            try:
                off = int(data) - base
                view = ws[off:off + 4 * int(count)].view(torch.float32)
                # order on the stream the engine names (include/d3f_hip.h: d3f_allreduce_fn), whatever torch's current is
                cur = torch.cuda.current_stream(dev)
                s = cur if int(stream or 0) == cur.cuda_stream else torch.cuda.ExternalStream(int(stream or 0), device=dev)
                with torch.cuda.stream(s):
                    dist.all_reduce(view, op=dist.ReduceOp.SUM, group=None if group is True else group)
                return 0
            except Exception as e:  # surfaces as the engine's error return (a raise cannot cross the C frame)
                err[0] = e
                return -3
        self._bn_cb = _lib.ALLREDUCE_FN(allreduce)  # kept alive with the engine
        check(L.d3f_unet_set_bn_sync(self.h, C.cast(self._bn_cb, C.c_void_p), None, int(world_size)))

    def flat_range(self, s0, s1, what):
        """[lo, hi): the flat gradient range that backward segments [s0, s1) write; refused unless it is one range"""
        segs = self.seg_ranges[s0:s1]
        lo, hi = min(b for b, _ in segs), max(e for _, e in segs)
        if sum(e - b for b, e in segs) != hi - lo:
            raise D3FError(f"{what}: segments {s0}..{s1 - 1} are not one contiguous flat range")
        return lo, hi

    def side_stream(self, device):
        """the engine's weight-gradient stream as a torch stream (None when the engine runs everything on the caller's
        stream); owned by the engine, valid as long as it lives"""
        if self._side is False:
            sp = C.c_void_p()
            check(_lib.lib().d3f_unet_side_stream(self.h, C.byref(sp)))
            self._side = torch.cuda.ExternalStream(sp.value, device=device) if sp.value else None
        return self._side

    def __del__(self):
        try:
            if self.h:
                _lib.lib().d3f_unet_destroy(self.h)
        except Exception:
            pass


def param_table(encoder_name, in_channels, classes):
    """[(name, shape, offset)] and BN table [(prefix, C, rm_off, rv_off)] from the C engine (host only)."""
    L = _lib.lib()
    h = C.c_void_p()
    check(L.d3f_unet_create(encoder_name.encode(), in_channels, classes, 1, 32, 32, _lib.F32, C.byref(h)))
    try:
        params, bns = [], []
        buf = C.create_string_buffer(256)
        shape = (C.c_int32 * 4)()
        nd, off = C.c_int(), C.c_int64()
        for i in range(L.d3f_unet_num_params(h)):
            check(L.d3f_unet_param_info(h, i, buf, 256, shape, C.byref(nd), C.byref(off)))
            params.append((buf.value.decode(), tuple(shape[k] for k in range(nd.value)), off.value))
        c, rm, rv = C.c_int(), C.c_int64(), C.c_int64()
        for i in range(L.d3f_unet_num_bn(h)):
            check(L.d3f_unet_bn_info(h, i, buf, 256, C.byref(c), C.byref(rm), C.byref(rv)))
            bns.append((buf.value.decode(), c.value, rm.value, rv.value))
        return params, bns, L.d3f_unet_param_floats(h), L.d3f_unet_bnstat_floats(h)
    finally:
        L.d3f_unet_destroy(h)


class _Lease:
    """marks an engine's workspace as holding the activations of a live autograd graph; released by the backward
    pass, or when the graph is dropped without one (the node, and with it this object, is destroyed)."""

    def __init__(self, engine):
        self.engine = engine
        engine.in_use = True

    def release(self):
        if self.engine is not None:
            self.engine.in_use = False
            self.engine = None

    __del__ = release


def _ptrs(ts):
    """a buffer argument of the C entry points: one network's pointer (d3f_unet_*) or the two networks' `T* const x[2]`
    array (d3f_unet_pair_*)"""
    return ptr(ts[0]) if len(ts) == 1 else ptr2(*ts)


def _float3(values):
    """a `const float v[3]` argument of the uint8 entries: a mean or a standard deviation per channel"""
    return (C.c_float * 3)(*[float(v) for v in values])


class _NetsFunction(torch.autograd.Function):
    """the autograd node of one recorded forward pass of `owner` (a Unet, or a UnetPair: one output per network)"""

    @staticmethod
    def forward(ctx, owner, engine, xs, *anchors):
        # `anchors`: ONE parameter per network that requires grad -- enough for autograd to record the node and call
        # backward, which writes every parameter's .grad itself; handing all 143 parameters to apply() cost ~0.15 ms of
        # host time per step
        ctx.owner, ctx.engine = owner, engine
        outs = owner._run_forward(engine, xs, training=True)
        ctx.serial = engine.serial
        ctx.lease = _Lease(engine)
        return outs

    @staticmethod
    def backward(ctx, *grad_outs):
        eng = ctx.engine
        if ctx.lease.engine is None:
            raise D3FError(f"backward through the d3f {type(ctx.owner).__name__} a second time: the activations were "
                           "released by the first backward (retain_graph is not supported by the HIP path)")
        if ctx.serial != eng.serial:
            # cannot happen through forward (a leased workspace is never handed out again); guards direct
            # _run_forward callers: silently using another forward's activations would give wrong gradients
            raise D3FError("the workspace of this forward pass was overwritten by a later forward before backward ran")
        # (autograd materialises the gradient of an output the loss does not depend on as zeros: that network's
        # parameter gradients then come out as exact zeros)
        ctx.owner._run_backward(eng, grad_outs)
        ctx.lease.release()
        return (None,) * len(ctx.needs_input_grad)  # every .grad was set by _run_backward (views of the flat gradient buffer)


class _NetsRuntime:
    """What runs a tuple of networks of one architecture as ONE set of launches -- `_nets`: (self,) for a Unet, (net_a,
    net_b) for a UnetPair: a pool of plans + workspaces per shape with their leases, the packed-weight stamp, the forward
    and backward enqueue with the data-parallel gradient buckets, and activation export.  The owner's `_rt` dict holds
    "engines" and "last_engine".  The number of networks only picks the C entry point: d3f_unet_* with one pointer per
    buffer, or d3f_unet_pair_* with two."""

    MAX_LIVE_GRAPHS = 4  # workspaces (2 GB each at bs 16, 256x256) per shape that may hold un-backwarded graphs

    def _engine(self, B, H, W, device):
        """a plan + workspace for this shape whose activations no live autograd graph still needs.  smp.Unet allows
        `crit(net(x1)) + crit(net(x2))` and a no_grad forward between forward and backward: each recorded forward
        leases its workspace until its backward has run, and a further forward of the same shape gets another one."""
        nets = self._nets
        a = nets[0]
        plan_nets = max(len(nets), getattr(a, "plan_nets", 1))  # (a pair plans for two networks whatever its nets say)
        key = (B, H, W, a.compute_dtype, device.index, plan_nets, a.activation)
        pool = self._rt["engines"].setdefault(key, [])
        for eng in pool:
            if not eng.in_use:
                return eng
        if len(pool) >= self.MAX_LIVE_GRAPHS:
            raise D3FError(f"{len(pool)} forward passes of shape {(B, H, W)} are waiting for their backward pass; "
                           f"run inference-only forwards under torch.no_grad()")
        eng = _Engine(a.encoder_name, a.in_channels, a.classes, B, H, W, a.compute_dtype, device, len(nets), plan_nets,
                      a.activation)
        if a._rt.get("bn_sync"):  # (a UnetPair refuses synchronised statistics before it gets here)
            eng.set_bn_sync(*a._rt["bn_sync"])
        pool.append(eng)
        return eng

    def _pack_if_needed(self, eng):
        # `p.data = view` keeps every parameter's OWN version counter, so in-place updates by
        # torch optimizers / load_state_dict show up on the parameters, not on the flat buffer
        nets = self._nets
        ver = tuple(n._weights_version() for n in nets)
        if eng.packed_version != ver:
            L = _lib.lib()
            args = (eng.h, _ptrs([n._rt["flat"] for n in nets]), ptr(eng.workspace), stream_ptr())
            check(L.d3f_unet_pack_weights(*args) if len(nets) == 1 else L.d3f_unet_pair_pack_weights(*args))
            eng.packed_version = ver

    def _forward_nets(self, xs):
        """the forward pass of the networks on xs (one input each, checked by the caller), recorded for autograd when a
        gradient is wanted"""
        nets = self._nets
        for net in nets:
            net._ensure_flat(xs[0].device)
        need = [torch.is_grad_enabled() and any(p.requires_grad for p in net._param_list) for net in nets]
        if any(need):
            if not all(need):
                raise D3FError("UnetPair: both networks (or neither) must require gradients")
            if not nets[0].training:
                raise D3FError("backward through an eval-mode Unet is not supported (BatchNorm is folded)")
            if any(x.requires_grad for x in xs):
                raise D3FError("gradient w.r.t. the network input is not computed by the HIP path")
        xs = tuple(x.detach().contiguous().float() for x in xs)
        eng = self._engine(xs[0].shape[0], xs[0].shape[2], xs[0].shape[3], xs[0].device)
        if not any(need):
            return self._run_forward(eng, xs, training=nets[0].training)
        return _NetsFunction.apply(self, eng, xs, *[next(p for p in net._param_list if p.requires_grad) for net in nets])

    def _run_forward(self, eng, xs, training):
        nets = self._nets
        self._pack_if_needed(eng)
        x = xs[0]
        outs = tuple(torch.empty((x.shape[0], nets[0].classes, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
                     for _ in nets)
        eng.serial += 1
        self._rt["last_engine"] = eng
        L = _lib.lib()
        args = (eng.h, _ptrs([n._rt["flat"] for n in nets]), _ptrs([n._rt["flat_bn"] for n in nets]), _ptrs(xs),
                _ptrs(outs), ptr(eng.workspace))
        if len(nets) == 1:
            check(L.d3f_unet_forward(*args, 1 if training else 0, stream_ptr()))
        else:  # train mode only (UnetPair checks it)
            check(L.d3f_unet_pair_forward(*args, stream_ptr()))
        if training:
            for net in nets:
                net._rt["flat_nbt"] += 1
        return outs

    def _backward_launch(self, eng, grad_outs, targets, s0, s1, join):
        """backward segments [s0, s1); join = 0: their gradients are final on the engine's side stream, not on this one"""
        nets = self._nets
        L = _lib.lib()
        args = (eng.h, _ptrs([n._rt["flat"] for n in nets]), _ptrs(grad_outs), _ptrs(targets), ptr(eng.workspace), s0, s1)
        if len(nets) == 1:
            check((L.d3f_unet_backward if join else L.d3f_unet_backward_nojoin)(*args, stream_ptr()))
        else:
            check(L.d3f_unet_pair_backward(*args, join, stream_ptr()))

    def _run_backward(self, eng, grad_outs):
        nets = self._nets
        grad_outs = [g.contiguous().float() for g in grad_outs]
        targets, directs = zip(*[net._backward_target() for net in nets])
        self._enqueue_backward(eng, grad_outs, targets, directs)
        for net, target, direct in zip(nets, targets, directs):
            net._publish_grads(target, direct)

    def _enqueue_backward(self, eng, grad_outs, targets, directs):
        nets = self._nets
        syncs = [net._rt["grad_sync"] for net in nets]
        if all(sync is None for sync in syncs):
            self._backward_launch(eng, grad_outs, targets, 0, eng.nseg, join=1)
            return
        # Data parallel: bucket k's collectives (one per network, each module's own reducer) must wait for bucket k's
        # gradients -- and nothing else may wait for anything.  The gradients become final on the engine's SIDE stream
        # (weight gradients run there; it also waits for this stream at the end of each bucket), so the hooks are called
        # with the side stream current: torch.distributed orders a collective behind the current stream at the time of
        # the call.  This stream (the dependent BatchNorm-backward -> data-gradient chain, the critical path) goes
        # straight on with bucket k+1; one join after the last bucket orders the optimiser behind the weight gradients.
        if any(sync is None for sync in syncs):
            raise D3FError("UnetPair: attach the data-parallel reducer to both networks or to neither")
        buckets = nets[0]._rt.get("grad_buckets")
        if any(net._rt.get("grad_buckets") != buckets for net in nets):
            raise D3FError("UnetPair: the two networks' gradient bucket settings differ")
        side = eng.side_stream(grad_outs[0].device)
        for k, (s0, s1) in enumerate(nets[0]._bucket_groups(buckets, eng.nseg)):
            self._backward_launch(eng, grad_outs, targets, s0, s1, join=0)
            lo, hi = eng.flat_range(s0, s1, f"gradient bucket {k}")
            with torch.cuda.stream(side):  # (a no-op for None, D3F_SERIAL_BACKWARD: everything is on this stream)
                for sync, target in zip(syncs, targets):
                    sync(k, target[lo:hi])
        check(_lib.lib().d3f_unet_backward_join(eng.h, stream_ptr()))

    def export_activation_shape(self, name):
        eng = self._rt.get("last_engine")
        if eng is None:
            raise D3FError("export_activation_shape() before any forward pass")
        dims = (C.c_int32 * 3)()
        check(_lib.lib().d3f_unet_export_shape(eng.h, name.encode(), dims))
        return (eng.shape[0], dims[0], dims[1], dims[2])

    def _export(self, net_index, name):
        eng = self._rt.get("last_engine")
        if eng is None:
            raise D3FError("export_activation() before any forward pass")
        out = torch.empty(self.export_activation_shape(name), dtype=torch.float32, device=eng.workspace.device)
        ws = C.c_void_p(eng.workspace.data_ptr() + int(net_index) * eng.net_stride)  # network 1: the pair's second copy
        check(_lib.lib().d3f_unet_export(eng.h, name.encode(), ws, ptr(out), stream_ptr()))
        return out


def _views_unverified(module, incompatible_keys):
    module._rt["verified"] = False


class Unet(nn.Module, _NetsRuntime):
    def __init__(self, encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=3,
                 activation=None, compute_dtype="f32"):
        """activation: a name of smp's Activation module, applied last to the head's convolution output in fp32 --
        None / "identity", "sigmoid", "tanh", "softmax2d" / "softmax", "logsoftmax", "clamp" (to [0, 1], smp's default
        bounds).  smp builds nn.Softmax() and nn.LogSoftmax() without `dim`, which torch resolves to dim=1 for a 4-D
        input: "softmax" and "logsoftmax" run over the channel axis, "softmax" is "softmax2d".  `self.activation` holds
        the canonical name ("identity" -> None, "softmax" -> "softmax2d").  "argmax" / "argmax2d" (integer output, no
        gradient) and callables (no device kernel) are refused."""
        super().__init__()
        if encoder_name not in _ENCODERS:
            raise KeyError(f"Wrong encoder name `{encoder_name}`, supported encoders: {list(_ENCODERS)}")
        if encoder_weights is not None:
            raise KeyError(f"Wrong pretrained weights `{encoder_weights}` for encoder `{encoder_name}`. "
                           f"Available options are: [None] (no network access)")
        self.activation = canonical_activation(activation)
        if compute_dtype not in _DTYPES:
            raise ValueError(f"compute_dtype must be one of f32 / f32x3 / bf16, got {compute_dtype}")
        self.encoder_name, self.in_channels, self.classes = encoder_name, in_channels, classes
        self.compute_dtype = _DTYPES[compute_dtype]
        self.plan_nets = 1  # set_plan_nets(2): this network's kernels are chosen as for a UnetPair (bit-identity runs)
        self.encoder = _Encoder(in_channels, _ENCODERS[encoder_name])
        self.decoder = _Decoder()
        self.segmentation_head = nn.Sequential(
            nn.Conv2d(16, classes, 3, padding=1), nn.Identity(),
            nn.Identity() if self.activation is None else _HeadActivation(self.activation))
        nn.init.xavier_uniform_(self.segmentation_head[0].weight)
        nn.init.constant_(self.segmentation_head[0].bias, 0)
        self._init_runtime_state()
        self.register_load_state_dict_post_hook(_views_unverified)  # (load_state_dict(assign=True) swaps Parameter objects)

    # -- runtime state that must not be deep-copied / pickled ------------------------------------
    def _init_runtime_state(self):
        self.__dict__["_rt"] = {"flat": None, "flat_grad": None, "flat_bn": None, "flat_nbt": None,
                                "engines": {}, "table": None, "gen": 0, "grad_sync": None, "params": None,
                                "bn_sync": None}

    def __deepcopy__(self, memo):
        rt = self.__dict__.pop("_rt")
        try:
            cls = self.__class__
            new = cls.__new__(cls)
            memo[id(self)] = new
            import copy
            for k, v in self.__dict__.items():
                new.__dict__[k] = copy.deepcopy(v, memo)
            new._init_runtime_state()
        finally:
            self.__dict__["_rt"] = rt
        return new

    def __getstate__(self):
        st = dict(self.__dict__)
        st.pop("_rt", None)
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self._init_runtime_state()

    # -- flat buffers -----------------------------------------------------------------------------
    def _table(self):
        rt = self._rt
        if rt["table"] is None:
            rt["table"] = param_table(self.encoder_name, self.in_channels, self.classes)
            names = [n for n, _ in self.named_parameters()]
            tnames = [n for n, _, _ in rt["table"][0]]
            if names != tnames:
                raise D3FError("parameter order of the module tree and of the C engine differ")
        return rt["table"]

    @property
    def _param_list(self):
        rt = self._rt
        if rt.get("params") is None:
            rt["params"] = [p for _, p in self.named_parameters()]
        return rt["params"]

    def _ensure_flat(self, device):
        """(re)establish: every parameter / BN buffer is a view into the flat device buffers."""
        rt = self._rt
        flat = rt["flat"]
        if rt.get("verified") and flat is not None and flat.device == device:
            # fast path (every forward comes through here: the full walk below costs ~0.9 ms of host time): the views were
            # verified once and nothing that re-homes parameter storage has run since -- nn.Module._apply (.to / .cuda /
            # .float ...) clears the flag; the first and last parameter and statistics views are still re-checked
            ps, bn = rt["params"], rt["flat_bn"]
            if ps[0].data_ptr() == flat.data_ptr() and ps[-1].data_ptr() + 4 * ps[-1].numel() == flat.data_ptr() + 4 * flat.numel() \
                    and rt["bn_first"].running_mean.data_ptr() == bn.data_ptr():
                return
        ptable, btable, nparam, nbn = self._table()
        named = dict(self.named_parameters())
        ok = flat is not None and flat.device == device
        if ok:
            base = flat.data_ptr()
            for name, shape, off in ptable:
                p = named[name]
                if p.data_ptr() != base + 4 * off or p.device != device:
                    ok = False
                    break
        if ok:
            bufs = dict(self.named_buffers())
            bb = rt["flat_bn"].data_ptr()
            for prefix, c, rm, rv in btable:
                if bufs[prefix + ".running_mean"].data_ptr() != bb + 4 * rm:
                    ok = False
                    break
        if ok:
            rt["verified"] = True
            rt["bn_first"] = dict(self.named_modules())[btable[0][0]]
            return
        flat = torch.empty(nparam, dtype=torch.float32, device=device)
        flat_bn = torch.empty(nbn, dtype=torch.float32, device=device)
        flat_nbt = torch.zeros(len(btable), dtype=torch.int64, device=device)
        with torch.no_grad():
            for name, shape, off in ptable:
                p = named[name]
                if tuple(p.shape) != tuple(shape):
                    raise D3FError(f"parameter {name}: shape {tuple(p.shape)} != engine {shape}")
                view = flat[off:off + p.numel()].view(shape)
                view.copy_(p.detach().to(device=device, dtype=torch.float32))
                p.data = view
            mods = dict(self.named_modules())
            for i, (prefix, c, rm, rv) in enumerate(btable):
                bn = mods[prefix]
                for attr, o in (("running_mean", rm), ("running_var", rv)):
                    view = flat_bn[o:o + c]
                    view.copy_(getattr(bn, attr).to(device=device, dtype=torch.float32))
                    setattr(bn, attr, view)
                flat_nbt[i] = bn.num_batches_tracked.to(device)
                bn.num_batches_tracked = flat_nbt[i]
        rt.update(flat=flat, flat_bn=flat_bn, flat_nbt=flat_nbt, flat_grad=None, grad_views=None, gen=rt.get("gen", 0) + 1,
                  params=[named[name] for name, _, _ in ptable], verified=True, bn_first=mods[btable[0][0]])
        for p in named.values():
            p.grad = None

    def set_plan_nets(self, plan_nets):
        """plan_nets = 2: every plan of this network makes the tile / split-K / slab / patch-kernel choices of a UnetPair
        (the workgroups of two networks counted together), so that stepping it alone computes bit for bit what the pair
        computes for it -- the reference side of the pair's bit-identity test.  Drops the existing plans."""
        if plan_nets not in (1, 2):
            raise ValueError("plan_nets must be 1 or 2")
        if plan_nets != getattr(self, "plan_nets", 1):
            self.plan_nets = plan_nets
            self._rt["engines"] = {}
            self._rt.pop("last_engine", None)
        return self

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .cpu() / .float() ...: torch replaces every parameter's storage -- the flat views are gone
        out = super()._apply(fn, *args, **kwargs)
        self._rt["verified"] = False
        return out

    def mark_params_changed(self):
        """call after writing the flat parameter buffer behind autograd's back (fused Adam / EMA)."""
        # a generation counter, not a flag: several plans (this network's own engines per shape, a UnetPair's engines)
        # hold packed copies of these weights and each compares its own stamp -- a flag cleared by whichever plan packed
        # first would leave the others on stale layouts
        self._rt["gen"] = self._rt.get("gen", 0) + 1

    @property
    def flat_params(self):
        return self._rt["flat"]

    @property
    def flat_grads(self):
        return self._rt["flat_grad"]

    @property
    def flat_bn_stats(self):
        return self._rt["flat_bn"]

    def prepare(self, device=None):
        """flatten parameters now (otherwise done lazily by the first forward); returns self."""
        device = torch.device(device) if device is not None else next(self.parameters()).device
        if device.type != "cuda":
            raise D3FError("d3f Unet runs on an MI355X (HIP) device only; there is no CPU fallback")
        self._ensure_flat(device)
        return self

    def set_sync_batchnorm(self, group=True, world_size=None):
        """Synchronised BatchNorm statistics over the ranks of `group` (True: the default process group; None: off = the
        default, per-GPU statistics -- what Lightning DDP does with the reference's Trainer flags).
        With it on, N ranks x bs are numerically one process with batch N*bs: every train-mode BatchNorm layer
        all-reduces its statistics in the forward pass and its two gradient sums in the backward pass (2 x 46 small
        collectives per step -- latency-bound, use it when batch statistics over bs/GPU images are too noisy)."""
        import torch.distributed as dist
        if group is not None:
            if not dist.is_initialized():
                raise D3FError("set_sync_batchnorm needs an initialised torch.distributed process group")
            world_size = world_size or dist.get_world_size(None if group is True else group)
        self._rt["bn_sync"] = None if group is None else (group, int(world_size))
        for pool in self._rt["engines"].values():
            for eng in pool:
                eng.set_bn_sync(*(self._rt["bn_sync"] or (None, 1)))

    def set_grad_sync(self, fn, buckets=2):
        """fn(bucket_index, flat_grad_slice) is called as soon as a gradient bucket is final
        (data-parallel all-reduce overlap); None disables.

        buckets: how the engine's backward segments (4: head + decoder | layer4 | layer3 | layer2 .. stem, final in that
        order) are grouped into exchange buckets -- None / 4: one bucket per segment; 2 (default, as DataParallel and
        bench.py: the machinery costs 1.3 % of a step against 3.2 % for 4): (head .. layer3: 92 MB, final at
        about two thirds of the backward pass) | (layer2 .. stem: 5.4 MB, the only bytes exchanged behind the backward
        pass); 1: one bucket = the whole gradient at the end of backward; or an explicit list of (first, end) segment
        ranges that tile range(nseg) in order.  Every bucket costs the chain a cross-stream event pair and RCCL a launch; fewer
        buckets expose more of the LAST bucket's all-reduce behind the backward pass."""
        self._rt["grad_sync"] = fn
        self._rt["grad_buckets"] = buckets

    @staticmethod
    def _bucket_groups(buckets, nseg):
        if isinstance(buckets, bool):
            raise D3FError(f"gradient buckets: {buckets!r} (a count 1 / 2 / {nseg}, None, or a list of segment ranges)")
        if buckets is None or buckets == nseg:
            return [(s, s + 1) for s in range(nseg)]
        if isinstance(buckets, int):
            if buckets == 1:
                return [(0, nseg)]
            if buckets == 2 and nseg >= 2:
                return [(0, nseg - 1), (nseg - 1, nseg)]
            raise D3FError(f"gradient buckets: {buckets} (the engine has {nseg} backward segments: 1, 2 or {nseg})")
        groups = [(int(b), int(e)) for b, e in buckets]
        if not groups or groups[0][0] != 0 or groups[-1][1] != nseg or any(b >= e for b, e in groups) or \
                any(groups[i][1] != groups[i + 1][0] for i in range(len(groups) - 1)):
            raise D3FError(f"gradient buckets {groups} do not tile the engine's {nseg} backward segments in order")
        return groups

    def set_early_update(self, fn):
        """fn(flat_grad, lo, hi) is called INSIDE backward, on the caller's stream behind the chain's last kernel and a
        wait for "the gradients of every bucket but the last are final" (flat range [lo, hi): layer3, layer4, decoder and
        head -- 94 % of the parameters), BEFORE the join with the side stream on which the last bucket's weight gradients
        (layer2, layer1, stem) are still running.  An optimiser that updates [lo, hi) in the hook runs next to that
        tail instead of behind it (FusedAdam(overlap_tail=True)).  Only
        taken when the gradients land in the flat buffer directly (every .grad None before backward) and no
        data-parallel reducer is attached; None disables."""
        self._rt["early_update"] = fn

    # -- engine -------------------------------------------------------------------------------------
    _nets = property(lambda self: (self,))

    def _weights_version(self):
        """stamp of the current parameter values: torch's version counters (in-place torch updates, load_state_dict) and the
        generation that mark_params_changed() bumps for raw-pointer updates (fused Adam, EMA lerp, re-homed buffers)"""
        rt = self._rt
        return (sum(p._version for p in rt["params"]) + rt["flat"]._version, rt.get("gen", 0))

    def _enqueue_backward(self, eng, grad_outs, targets, directs):
        early = self._rt.get("early_update")
        side = eng.side_stream(grad_outs[0].device) if (early is not None and self._rt["grad_sync"] is None and directs[0]
                                                       and eng.nseg > 1) else None
        if side is None:
            return super()._enqueue_backward(eng, grad_outs, targets, directs)
        # every bucket is enqueued without a join; the leading buckets' gradients are final on the side stream at the
        # event, and the hook's update runs on THIS stream behind the chain's last kernel -- next to the last bucket's
        # weight gradients, which are still running on the side stream -- before the join that step() would wait for
        last = eng.nseg - 1
        lo, hi = eng.flat_range(0, last, "early update")
        self._backward_launch(eng, grad_outs, targets, 0, last, join=0)
        final = side.record_event()
        self._backward_launch(eng, grad_outs, targets, last, eng.nseg, join=0)
        torch.cuda.current_stream().wait_event(final)
        early(targets[0], lo, hi)
        check(_lib.lib().d3f_unet_backward_join(eng.h, stream_ptr()))

    def _backward_target(self):
        """(flat buffer the engine writes this pass's gradients into, direct): direct = every .grad is None, the gradients
        land in the module's own flat gradient buffer and the parameters' .grad become views of it"""
        rt = self._rt
        direct = all(p.grad is None for p in self._param_list)
        if rt["flat_grad"] is None:
            rt["flat_grad"] = torch.empty_like(rt["flat"])
            rt["grad_views"] = None
        rt["backward_calls"] = rt.get("backward_calls", 0) + 1
        return (rt["flat_grad"] if direct else torch.empty_like(rt["flat"])), direct

    def _publish_grads(self, target, direct):
        rt = self._rt
        params = self._param_list
        ptable = self._table()[0]
        if direct:
            # the same 143 view tensors of the flat gradient buffer every step (making them anew cost ~0.3 ms of host time)
            views = rt.get("grad_views")
            if views is None or views[0].data_ptr() != target.data_ptr():
                views = rt["grad_views"] = [target[off:off + p.numel()].view(shape) for (_, shape, off), p in zip(ptable, params)]
            for p, view in zip(params, views):
                if p.requires_grad:
                    p.grad = view
            return
        for (name, shape, off), p in zip(ptable, params):
            if not p.requires_grad:
                continue
            view = target[off:off + p.numel()].view(shape)
            if p.grad is None:
                p.grad = view.clone()
            else:
                p.grad.add_(view)

    # -- nn.Module API ------------------------------------------------------------------------------
    def check_input_shape(self, x):
        h, w = x.shape[-2:]
        if h % 32 != 0 or w % 32 != 0:
            new_h = (h // 32 + 1) * 32 if h % 32 != 0 else h
            new_w = (w // 32 + 1) * 32 if w % 32 != 0 else w
            raise RuntimeError(
                f"Wrong input shape height={h}, width={w}. Expected image height and width divisible by 32. "
                f"Consider pad your images to shape ({new_h}, {new_w}).")

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"Expected input [B, {self.in_channels}, H, W], got {list(x.shape)}")
        self.check_input_shape(x)
        if x.device.type != "cuda":
            raise D3FError("d3f Unet runs on an MI355X (HIP) device only; there is no CPU fallback "
                           "(input tensor is on %s)" % x.device)
        return self._forward_nets((x,))[0]

    @torch.no_grad()
    def forward_graph(self, x, out=None):
        """Eval-mode forward replayed from a hipGraph (BASELINE.json configs[4]: "hipGraph-captured denoise step"; the
        reference's frame loop is d3f/script_tools/put_video_through_fake_model.py:111-119).  The graph is captured on
        the first call per (x, out) buffer pair and bakes those pointers in, so a sampling loop passes the SAME two
        buffers every iteration (write the next input into `x` in place); results are bit-identical to `self(x)` in
        eval mode.  Parameter updates between calls are picked up (values are read at replay time)."""
        if self.training:
            raise D3FError("forward_graph is the eval-mode (BatchNorm folded) forward: call .eval() first")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"Expected input [B, {self.in_channels}, H, W], got {list(x.shape)}")
        self.check_input_shape(x)
        if x.device.type != "cuda":
            raise D3FError("d3f Unet runs on an MI355X (HIP) device only; there is no CPU fallback")
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("forward_graph bakes the input pointer into the graph: pass a contiguous float32 tensor")
        shape = (x.shape[0], self.classes, x.shape[2], x.shape[3])
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=x.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on the input's device")
        self._ensure_flat(x.device)
        eng = self._engine(x.shape[0], x.shape[2], x.shape[3], x.device)
        self._pack_if_needed(eng)
        rt = self._rt
        eng.serial += 1
        rt["last_engine"] = eng
        check(_lib.lib().d3f_unet_forward_graph(eng.h, ptr(rt["flat"]), ptr(rt["flat_bn"]), ptr(x), ptr(out),
                                                ptr(eng.workspace), stream_ptr()))
        eng.keep_graph = (x, out)  # the captured graph holds these pointers: keep them alive with the engine
        return out

    @torch.no_grad()
    def predict_u8(self, frames_bgr, mean, std, graph=True, out=None):
        """Inference on uint8 BGR frames ([H,W,3] or [B,H,W,3] on the HIP device) -> uint8 BGR frames.

        Eval-mode forward (BatchNorm running statistics folded into the conv epilogues) with the reference's
        `cv2_to_tensor_normalised` / `tensor_cv2_to_denormalised` (d3f/train_deep_fake/lit_module.py:272-300) fused
        into the first and last kernel; `graph=True` replays a hipGraph captured per (input, output) buffer pair,
        so pass the same buffers again (`out=`) in a frame loop."""
        x, single = self._u8_batch(frames_bgr, "predict_u8", "H, W")
        x = x.contiguous()
        B, H, W, _ = x.shape
        self._check_u8_size(H, W)
        eng = self._u8_engine(B, H, W, x.device)
        if out is None:
            out = torch.empty_like(x)
        elif out.shape != x.shape or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 tensor shaped like the input batch")
        rt = self._rt
        check(_lib.lib().d3f_unet_predict_u8(eng.h, ptr(rt["flat"]), ptr(rt["flat_bn"]), ptr(x), ptr(out), _float3(mean),
                                             _float3(std), ptr(eng.workspace), 1 if graph else 0, stream_ptr()))
        eng.keep = (x, out)  # the captured graph bakes these pointers in: keep them alive with the engine
        return out[0] if single else out

    # -- what the uint8 entries share ------------------------------------------------------------------
    @staticmethod
    def _u8_batch(frames, who, dims):
        """the frames of the uint8 entry `who`, checked -> (the batch [B, ., ., 3], whether one frame [., ., 3] came in)"""
        if frames.dtype != torch.uint8 or frames.shape[-1] != 3 or frames.dim() not in (3, 4):
            raise ValueError(f"{who} expects uint8 frames [{dims}, 3] or [B, {dims}, 3] in BGR order")
        if frames.device.type != "cuda":
            raise D3FError(f"{who} needs frames on the HIP device (no CPU fallback)")
        single = frames.dim() == 3
        return (frames.unsqueeze(0) if single else frames), single

    @staticmethod
    def _check_u8_size(H, W):
        if H % 32 or W % 32:
            raise RuntimeError(f"Wrong input shape height={H}, width={W}. Expected image height and width "
                               f"divisible by 32.")

    def _u8_engine(self, B, H, W, device):
        """the plan for B frames at the network size H x W, its weights packed"""
        self._ensure_flat(device)
        eng = self._engine(B, H, W, device)
        self._pack_if_needed(eng)
        return eng

    def _frame_inputs(self, who, raw_bgr, size, pair, pair_name, in_place=False, boxes=None):
        """what the two raw-frame entries do before their C call -> (contiguous frames [B, h, w, 3], single, the call's
        geometry, the plan, the pair buffer [B, H, 2W, 3]: `pair`, checked, or a new one, the call's boxes as a list).
        The geometry is (h, w, x1, y1, cw, ch) -- the centre-crop box for boxes=None, or the one box boxes names with 4
        integers -- or, for boxes [B][4], (h, w, table) with the host int32 table the boxes entries take."""
        from . import ops
        x, single = self._u8_batch(raw_bgr, who, "h, w")
        if in_place and not x.is_contiguous():
            raise ValueError("out=raw_bgr (in place) needs contiguous frames")
        x = x.contiguous()
        B, h, w, _ = x.shape
        H, W = int(size[0]), int(size[1])
        self._check_u8_size(H, W)
        if boxes is None:
            rows = [tuple(ops.center_crop_box(h, w, W, H))]
            geo = (h, w) + rows[0]
        else:
            if isinstance(boxes, torch.Tensor):
                boxes = boxes.tolist()
            boxes = list(boxes)
            if len(boxes) == 4 and not any(hasattr(v, "__len__") for v in boxes):  # one box for every frame
                rows = [tuple(int(v) for v in boxes)]
                geo = (h, w) + rows[0]
            else:
                table, rows = ops._boxes_arg(boxes, B, who)
                geo = (h, w, table)
        eng = self._u8_engine(B, H, W, x.device)
        shape = (B, H, 2 * W, 3)
        if pair is None:
            pair = torch.empty(shape, dtype=torch.uint8, device=x.device)
        elif tuple(pair.shape) != shape or pair.dtype != torch.uint8 or not pair.is_contiguous() or pair.device != x.device:
            raise ValueError(f"{pair_name} must be a contiguous uint8 tensor of shape {shape} on the input's device")
        return x, single, geo, eng, pair, rows

    @staticmethod
    def _frame_rot(who, angles, boxes, raw_bgr, antialias, multiband=False):
        """angles= of the two raw-frame entries -> the host int32 table [B][2] the rboxes entries take, or None for the
        axis-aligned call (angles None, or all zero after rounding to hundredths).  Checked before anything touches the
        device"""
        from . import ops
        if angles is None:
            return None
        rows = boxes.tolist() if isinstance(boxes, torch.Tensor) else (None if boxes is None else list(boxes))
        if rows is None or (len(rows) == 4 and not any(hasattr(v, "__len__") for v in rows)):
            raise ValueError(f"{who}: angles= needs boxes= with a box per frame")
        rot = ops._rot_arg(angles, 1 if raw_bgr.dim() == 3 else int(raw_bgr.shape[0]), who)
        if rot is not None and antialias:
            raise ValueError(f"{who}: antialias=True with non-zero angles: the antialiased crop of a rotated box is out of "
                             f"scope")
        if rot is not None and multiband:
            raise ValueError(f"{who}: blend='multiband' with non-zero angles: the multiband pyramid of a rotated box is out "
                             f"of scope")
        return rot

    @staticmethod
    def _apply_frame_settings(eng, antialias, color, temporal, blend=None):
        """the frame entries' settings on the plan's handle, in front of every call (the handle returns early on a value it
        already has, and keeps its captured graphs and the filter's state then).  color: a D3F_COLOR_* code, or None: left
        as it is -- `predict_frames_u8` has no paste to colour.  temporal: what `_lib.temporal_setting` returns.  blend:
        (D3F_BLEND_* code, levels), or None: left as it is, for the same reason."""
        L = _lib.lib()
        check(L.d3f_unet_set_frame_resample(eng.h, _lib.RESAMPLE_CUBIC_AA if antialias else _lib.RESAMPLE_CUBIC))
        if color is not None:
            check(L.d3f_unet_set_frame_color_match(eng.h, color))
        if blend is not None:
            check(L.d3f_unet_set_frame_blend(eng.h, blend[0], blend[1]))
        check(L.d3f_unet_set_frame_temporal(eng.h, temporal[0], temporal[1]))

    def reset_frame_temporal(self):
        """forget the temporal filter's past on every plan of this network: the next frame of `predict_frames_u8` /
        `predict_frames_full_u8` with `temporal=` is a first frame again (d3f_unet_frame_temporal_reset, on the current
        stream; captured graphs stay)"""
        # (every plan in a Unet's pools is a single network's, and one that never had the filter on has nothing to forget)
        for pool in self._rt.get("engines", {}).values():
            for eng in pool:
                check(_lib.lib().d3f_unet_frame_temporal_reset(eng.h, stream_ptr()))

    @torch.no_grad()
    def predict_frames_u8(self, raw_bgr, size, mean, std, graph=True, out=None, antialias=False, temporal=None,
                          boxes=None, angles=None):
        """The frame path of d3f/script_tools/put_video_through_fake_model.py:111-119, 68 on decoded frames of any
        size: uint8 BGR frames [h,w,3] or [B,h,w,3] on the HIP device -> centre crop to the aspect of size = (H, W)
        (`ops.center_crop_box`) -> bicubic resize (`ops.crop_resize_cubic_u8`) -> `predict_u8` -> the real|fake frames
        [B,H,2W,3] ([H,2W,3] for a single frame), all in one C call.  The left half is byte for byte
        `ops.crop_resize_cubic_u8`, the right half `predict_u8` of the left half at the same batch size.  `graph=True`
        replays a hipGraph captured per (input, output) buffer pair, raw frame size and crop box: pass the same buffers
        again (`out=`) in a frame loop.  antialias=True resizes as `ops.crop_resize_cubic_u8(..., antialias=True)` does
        (the handle's D3F_RESAMPLE_CUBIC_AA mode); a change of it between calls re-captures the graph.
        temporal: None (off), a strength in (0, 1) or (strength, threshold): the fake half is filtered against flicker
        (`ops.temporal_filter_u8` with real = the left half, fake = the right half; d3f_unet_set_frame_temporal).  The
        frames of successive calls are then consecutive in time, the state lives with the plan of this batch size and
        network size, `reset_frame_temporal()` starts a new sequence, and a change of the values starts one too.
        boxes: None is the centre crop.  One box (x1, y1, cw, ch) is that box for every frame, through the same C entry, with
        `graph=` honoured (the box is part of the graph's key).  [B][4] integers in host memory are a box per frame -- a
        face that moves (`ops.track_crop_box`) -- through d3f_unet_predict_frames_boxes_u8: still one C call, the left half
        byte for byte `ops.crop_resize_cubic_u8(..., boxes=)`, and it runs EAGER whatever `graph=` says: a captured launch
        bakes the boxes in, so a moving box would re-capture on every call.  The temporal filter reads the resized crop: a
        box that moves is motion to it.
        angles: B angles in degrees next to a box per frame -- a head that rolls (`ops.box_rotation`) -- through
        d3f_unet_predict_frames_rboxes_u8: the left half is byte for byte `ops.crop_resize_cubic_u8(..., boxes=, angles=)`.
        None, or all zero after rounding to hundredths, is the boxes= call.  Not with antialias=True."""
        temporal = _lib.temporal_setting(temporal)
        rot = self._frame_rot("predict_frames_u8", angles, boxes, raw_bgr, antialias)
        x, single, geo, eng, out, _ = self._frame_inputs("predict_frames_u8", raw_bgr, size, out, "out", boxes=boxes)
        rt = self._rt
        self._apply_frame_settings(eng, antialias, None, temporal)
        L = _lib.lib()
        per_frame = len(geo) == 3
        entry = L.d3f_unet_predict_frames_boxes_u8 if per_frame else L.d3f_unet_predict_frames_u8
        if rot is not None:
            entry, geo = L.d3f_unet_predict_frames_rboxes_u8, geo + (rot,)
        check(entry(eng.h, ptr(rt["flat"]), ptr(rt["flat_bn"]), ptr(x), *geo, ptr(out), _float3(mean), _float3(std),
                    ptr(eng.workspace), 1 if graph and not per_frame else 0, stream_ptr()))
        eng.keep = (x, out)  # the captured graph bakes these pointers in: keep them alive with the engine
        return out[0] if single else out

    @torch.no_grad()
    def predict_frames_full_u8(self, raw_bgr, size, mean, std, feather=None, graph=True, out=None, pair_out=None,
                               antialias=False, color_match=None, temporal=None, boxes=None, blend=None,
                               blend_levels=None, angles=None):
        """`predict_frames_u8`, then the fake pasted back into the source frames: uint8 BGR frames [h,w,3] or [B,h,w,3] on
        the HIP device -> the frames at their own size with the centre-crop box replaced by the fake, resized back
        (`ops.paste_resize_cubic_u8`) and blended in over `feather` source pixels (None: `ops.default_feather` of the
        box), all in one C call.  Returns the full frames.  pair_out: a [B,H,2W,3] buffer, filled as `predict_frames_u8`
        fills it (allocated when None: it stages the fake).  out=raw_bgr pastes in place (graph=False only).  `graph=True`
        replays a hipGraph of its own, captured per set of buffers, frame size, box and feather.  antialias: as
        `predict_frames_u8`, for the crop-to-network resize only; the paste enlarges and stays as it is.
        color_match: None / "none", or "meanstd": the fake's mean and standard deviation are matched to the resized real
        crop's, per frame and channel, before the paste (`ops.channel_sums_u8` of both halves of the pair,
        `ops.color_match_coef`, `ops.paste_resize_cubic_u8(..., color=)`, still in the one C call; the handle's
        D3F_COLOR_MEANSTD mode).  pair_out is not touched by it; a change between calls re-captures the graph.
        temporal: as `predict_frames_u8` -- the fake half of pair_out is filtered before the sums and the paste read it,
        and with color_match="meanstd" the coefficients are smoothed across frames too (`ops.color_coef_smooth`).
        boxes: as `predict_frames_u8` -- None, one box (the same C entry, `graph=` honoured) or [B][4], a box per frame
        (d3f_unet_predict_frames_full_boxes_u8: eager whatever `graph=` says); every frame's fake is pasted into its own
        box, with one feather for the call: None is `ops.default_feather(min cw, min ch)` over the call's boxes.
        blend: None / "feather": the single ramp above.  "multiband": the paste is `ops.paste_multiband_u8` on the fake half
        of the pair instead (with color_match its colour form, with boxes its boxes form), still in the one C call (the
        handle's D3F_BLEND_MULTIBAND mode; its pyramid workspace belongs to the plan and grows with the box): low frequencies
        fade over `feather` pixels, fine detail over a fraction of it.  blend_levels: the pyramid's levels, 1..6, with
        "multiband" only; None: `ops.multiband_levels(feather)`.  A change of either re-captures the graph.
        angles: as `predict_frames_u8` (d3f_unet_predict_frames_full_rboxes_u8): every frame's fake is pasted into its own
        rotated rectangle (`ops.paste_resize_cubic_u8(..., boxes=, angles=)`).  Not with antialias=True or
        blend="multiband"."""
        from . import ops
        blend_code = _lib.blend_mode(blend)
        if blend_levels is not None and blend_code != _lib.BLEND_MULTIBAND:
            raise ValueError("blend_levels needs blend='multiband'")
        if blend_levels is not None:
            blend_levels = _lib.blend_levels(blend_levels)
        color_code = _lib.color_match_mode(color_match)
        temporal = _lib.temporal_setting(temporal)
        in_place = out is raw_bgr
        rot = self._frame_rot("predict_frames_full_u8", angles, boxes, raw_bgr, antialias, blend_code == _lib.BLEND_MULTIBAND)
        x, single, geo, eng, pair_out, rows = self._frame_inputs("predict_frames_full_u8", raw_bgr, size, pair_out,
                                                                 "pair_out", in_place, boxes=boxes)
        if feather is None:
            feather = ops.default_feather(min(row[2] for row in rows), min(row[3] for row in rows))
        feather = int(feather)
        if in_place:
            full = x
        elif out is None:
            full = torch.empty_like(x)
        else:
            full = out.unsqueeze(0) if single and out.dim() == 3 else out
            if (tuple(full.shape) != tuple(x.shape) or full.dtype != torch.uint8 or not full.is_contiguous()
                    or full.device != x.device):
                raise ValueError(f"out must be a contiguous uint8 tensor of shape {tuple(raw_bgr.shape)} on the input's device")
        rt = self._rt
        if blend_code == _lib.BLEND_MULTIBAND and blend_levels is None:
            blend_levels = ops.multiband_levels(feather)
        self._apply_frame_settings(eng, antialias, color_code, temporal, (blend_code, blend_levels or 1))
        L = _lib.lib()
        per_frame = len(geo) == 3
        entry = L.d3f_unet_predict_frames_full_boxes_u8 if per_frame else L.d3f_unet_predict_frames_full_u8
        if rot is not None:
            entry, geo = L.d3f_unet_predict_frames_full_rboxes_u8, geo + (rot,)
        check(entry(eng.h, ptr(rt["flat"]), ptr(rt["flat_bn"]), ptr(x), *geo, feather, ptr(pair_out), ptr(full),
                    _float3(mean), _float3(std), ptr(eng.workspace), 1 if graph and not per_frame else 0, stream_ptr()))
        eng.keep_full = (x, pair_out, full)  # the captured graph bakes these pointers in: keep them alive with the engine
        return full[0] if single else full

    def export_activation(self, name):
        """debugging / parity tests: an internal tensor of the MOST RECENT forward (+ backward) as NCHW f32 --
        "<conv name>:y" raw conv output, ":a" post BatchNorm(+residual)+ReLU activation, ":da" gradient w.r.t. that
        activation (d3f_unet_export).  Channels beyond the real count (vector padding) are cut off by the caller."""
        return self._export(0, name)

    # flops of the conv contractions of one call (2*MAC), for roofline reporting
    def conv_flops(self, B, H, W, device=None):
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        eng = self._engine(B, H, W, device)
        return eng.fwd_flops, eng.bwd_flops


# ---------------------------------------------------------------------------------------------
# two networks, one set of launches
# ---------------------------------------------------------------------------------------------
class UnetPair(_NetsRuntime):
    """Two `Unet`s of identical architecture stepped as ONE set of kernel launches.

    train_deep_fake's `mode: "denoise"` trains model_a on domain a and model_b on domain b with nothing shared
    (d3f/train_deep_fake/lit_module.py:142-181): two independent forward / backward passes of 8 images each per batch, every
    launch half-filling the chip.  `UnetPair(model_a, model_b)(xa, xb)` runs both networks' layer k as one launch
    (libd3f_hip.so: d3f_unet_pair_forward / d3f_unet_pair_backward -- gridDim.z carries the network) with the tile choices
    of a 16-image batch, and returns (prediction_a, prediction_b) wired into autograd: ONE backward pass fed both output
    gradients, `torch.autograd.backward([loss_a, loss_b])`, writes both networks' .grad.  The two modules keep their own
    parameters, gradients, BatchNorm statistics and optimisers; values are bit for bit those of each network stepped alone
    with `Unet.set_plan_nets(2)`.  Train mode, per-GPU BatchNorm statistics."""

    def __init__(self, net_a, net_b):
        if not (isinstance(net_a, Unet) and isinstance(net_b, Unet)) or net_a is net_b:
            raise TypeError("UnetPair takes two distinct d3f Unet modules")
        for attr in ("encoder_name", "in_channels", "classes", "compute_dtype", "activation"):
            if getattr(net_a, attr) != getattr(net_b, attr):
                raise ValueError(f"UnetPair: the two networks differ in {attr}")
        self.nets = (net_a, net_b)
        self._rt = {"engines": {}}

    _nets = property(lambda self: self.nets)
    _engines = property(lambda self: self._rt["engines"])  # plans + workspaces per shape (what tests and tools read)
    last_engine = property(lambda self: self._rt.get("last_engine"))  # the plan of the most recent pair pass

    # plans and workspaces are runtime state (C handles): a copy / pickle of whatever holds the pair starts without them
    def __deepcopy__(self, memo):
        import copy
        return UnetPair(copy.deepcopy(self.nets[0], memo), copy.deepcopy(self.nets[1], memo))

    def __getstate__(self):
        return {"nets": self.nets}

    def __setstate__(self, st):
        self.nets = st["nets"]
        self._rt = {"engines": {}}

    def usable(self, xa, xb):
        """can this batch go through the pair?  Same shape, both networks training on one HIP device, and neither with
        synchronised BatchNorm statistics (the pair engine keeps per-GPU statistics)"""
        a, b = self.nets
        return (xa.shape == xb.shape and xa.device == xb.device and xa.device.type == "cuda" and a.training and b.training
                and not a._rt.get("bn_sync") and not b._rt.get("bn_sync"))

    def __call__(self, xa, xb):
        a, b = self.nets
        if xa.shape != xb.shape or xa.dim() != 4 or xa.shape[1] != a.in_channels:
            raise RuntimeError(f"UnetPair expects two inputs of one shape [B, {a.in_channels}, H, W], got "
                               f"{list(xa.shape)} and {list(xb.shape)}")
        a.check_input_shape(xa)
        if xa.device.type != "cuda" or xb.device != xa.device:
            raise D3FError("d3f UnetPair runs on one MI355X (HIP) device; there is no CPU fallback")
        if not (a.training and b.training):
            raise D3FError("UnetPair runs the train-mode passes of train_deep_fake's denoise step; eval-mode inference "
                           "goes through each Unet")
        if a._rt.get("bn_sync") or b._rt.get("bn_sync"):
            raise D3FError("UnetPair keeps per-GPU BatchNorm statistics; switch set_sync_batchnorm off or step the networks alone")
        return self._forward_nets((xa, xb))

    def export_activation(self, net_index, name):
        """`Unet.export_activation` for network 0 / 1 of the most recent pair pass"""
        return self._export(net_index, name)
