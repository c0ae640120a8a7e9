"""CPU: the C-ABI library loads, exports every symbol include/d3f_hip.h declares, and its host-side
planning (no compute, no GPU) agrees with the module tree and the survey's analytic figures."""
import ctypes as C

import pytest
import torch

from denoising_diffusion_deep_fake_amd import _lib


def test_library_exports_every_declared_symbol():
    lib = _lib.lib()
    declared = _lib.header_symbols()
    assert len(declared) >= 40
    assert set(declared) == set(_lib.PROTOTYPES), set(declared) ^ set(_lib.PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.d3f_version() >= 100


def test_plan_matches_survey_figures():
    lib = _lib.lib()
    h = C.c_void_p()
    _lib.check(lib.d3f_unet_create(b"resnet34", 3, 3, 16, 256, 256, _lib.F32, C.byref(h)))
    try:
        assert lib.d3f_unet_param_floats(h) == 24_436_659
        assert lib.d3f_unet_num_params(h) == 140 and lib.d3f_unet_num_bn(h) == 46
        assert lib.d3f_unet_bnstat_floats(h) == 2 * 9504
        # SURVEY.md 8d / BASELINE.md: 15.666 GFLOP forward, 46.689 GFLOP per trained image at 256x256
        fwd = lib.d3f_unet_forward_flops(h) / 16 / 1e9
        bwd = lib.d3f_unet_backward_flops(h) / 16 / 1e9
        assert abs(fwd - 15.666) < 1e-3 and abs(fwd + bwd - 46.689) < 2e-3
        assert lib.d3f_unet_num_segments(h) == 4
        prev_begin = None
        total = 0
        for s in range(4):
            b, e = C.c_int64(), C.c_int64()
            _lib.check(lib.d3f_unet_segment_range(h, s, C.byref(b), C.byref(e)))
            assert b.value < e.value
            if prev_begin is not None:
                assert e.value == prev_begin  # buckets tile the flat gradient back to front
            prev_begin = b.value
            total += e.value - b.value
        assert prev_begin == 0 and total == 24_436_659
        assert lib.d3f_unet_workspace_bytes(h) > 2**30
    finally:
        lib.d3f_unet_destroy(h)


def test_plan_errors_mirror_smp():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.d3f_unet_create(b"resnet34", 3, 3, 2, 48, 64, _lib.F32, C.byref(h)) != 0
    assert b"divisible by 32" in lib.d3f_last_error()
    assert lib.d3f_unet_create(b"vgg16", 3, 3, 2, 64, 64, _lib.F32, C.byref(h)) != 0
    assert b"Wrong encoder name" in lib.d3f_last_error()


def test_pair_handle_refuses_the_single_network_calls():
    """a pair handle (d3f_unet_create_nets(..., nets = 2, ...)) is refused by predict_u8, forward_graph, train_step and
    set_bn_sync with a callback before anything reaches a device -- the dummy pointers below are never dereferenced;
    removing a callback still succeeds.  Host only: with a device visible, a library without the guard would launch."""
    if torch.cuda.is_available():
        pytest.skip("host-only check of the C ABI guards (dummy device pointers)")
    from denoising_diffusion_deep_fake_amd.graph_step import StepBuffers
    lib = _lib.lib()
    h = C.c_void_p()
    _lib.check(lib.d3f_unet_create_nets(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, 2, 2, C.byref(h)))
    try:
        d = C.c_void_p(0x1000)
        mean_std = (C.c_float * 3)(0.5, 0.5, 0.5)
        buffers = StepBuffers(*[0x1000] * len(StepBuffers._fields_))
        callback = _lib.ALLREDUCE_FN(lambda ctx, data, count, stream: 0)
        calls = {
            "predict_u8": lambda: lib.d3f_unet_predict_u8(h, d, d, d, d, mean_std, mean_std, d, 0, None),
            "forward_graph": lambda: lib.d3f_unet_forward_graph(h, d, d, d, d, d, None),
            "train_step": lambda: lib.d3f_unet_train_step(h, C.byref(buffers), 5.0, -1.0, 1.0, d, 0, None),
            "set_bn_sync": lambda: lib.d3f_unet_set_bn_sync(h, C.cast(callback, C.c_void_p), None, 2),
        }
        for name, call in calls.items():
            assert call() != 0, name
            assert b"pair" in lib.d3f_last_error(), (name, lib.d3f_last_error())
        assert lib.d3f_unet_set_bn_sync(h, None, None, 1) == 0
    finally:
        lib.d3f_unet_destroy(h)


def test_module_tree_matches_engine_table_and_oracle_keys():
    import oracle
    from denoising_diffusion_deep_fake_amd import Unet
    from denoising_diffusion_deep_fake_amd.unet import param_table
    net = Unet("resnet34", None, 3, 3, None)
    params, bns, nparam, nbn = param_table("resnet34", 3, 3)
    assert [n for n, _ in net.named_parameters()] == [n for n, _, _ in params]
    assert all(tuple(p.shape) == s for (_, p), (_, s, _) in zip(net.named_parameters(), params))
    assert all(off % 4 == 0 for _, _, off in params)  # 16-byte aligned views
    ref = oracle.Unet("resnet34", None, 3, 3, None)
    assert list(ref.state_dict().keys()) == list(net.state_dict().keys())
    mods = dict(net.named_modules())
    assert all(isinstance(mods[p], torch.nn.BatchNorm2d) and mods[p].num_features == c for p, c, _, _ in bns)
    r18 = Unet("resnet18", None, 3, 3, None)
    assert sum(p.numel() for p in r18.parameters()) == param_table("resnet18", 3, 3)[2]


def test_no_cpu_fallback():
    from denoising_diffusion_deep_fake_amd import D3FError, Unet, ops
    with pytest.raises(D3FError):
        Unet("resnet34", None, 3, 3, None)(torch.zeros(1, 3, 32, 32))
    with pytest.raises(D3FError):
        ops.mse_ssim_loss(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32))


def test_conv_descriptor_validation_on_host():
    lib = _lib.lib()
    d = _lib.ConvDesc(2, 16, 16, 6, 0, 0, 8, 3, 3, 1, 1, 6)  # C0 = 6 not a multiple of 4
    assert lib.d3f_conv_packed_bytes(_lib.F32, C.byref(d), 0) == 0
    assert b"multiples of 4" in lib.d3f_last_error()
    d = _lib.ConvDesc(2, 16, 16, 64, 0, 0, 128, 3, 3, 2, 1, 64)
    assert lib.d3f_conv_packed_bytes(_lib.F32, C.byref(d), 0) == 128 * 576 * 4
    tiles = C.c_int()
    assert lib.d3f_conv_stats_floats(_lib.F32, C.byref(d), 0, C.byref(tiles)) == tiles.value * 128 * 2
    assert lib.d3f_conv_workspace_bytes(_lib.F32, C.byref(d), 0) > 0  # 128 rows x 128 channels: split-K


def test_conv_pack_weights_refuses_a_layer_beyond_the_packing_table():
    """d3f_conv_pack_weights packs through the network's table-driven kernel (16-bit extents, 32-bit element indices): a
    layer beyond that range is refused with an error that names the limit before anything is launched -- the dummy
    pointers below are never dereferenced -- while d3f_conv_packed_bytes still sizes it."""
    if torch.cuda.is_available():
        pytest.skip("host-only check of the C ABI guard (dummy device pointers)")
    lib = _lib.lib()
    d = _lib.ConvDesc(1, 8, 8, 8192, 0, 0, 64, 3, 3, 1, 1, 8192)  # Kpad = 9 x 8192 = 73728
    p = C.c_void_p(0x1000)
    for dtype, wsz in ((_lib.F32, 4), (_lib.BF16, 2), (_lib.F32X3, 6)):
        assert lib.d3f_conv_packed_bytes(dtype, C.byref(d), 0) == 64 * 73728 * wsz
        assert lib.d3f_conv_packed_bytes(dtype, C.byref(d), 1) == 8192 * 576 * wsz
        for w_fwd, w_dgrad in ((p, p), (p, None), (None, p)):
            assert lib.d3f_conv_pack_weights(dtype, C.byref(d), p, w_fwd, w_dgrad, None) != 0
            err = lib.d3f_last_error()
            assert b"packing table" in err and b"65536" in err, err


def test_library_digest_matches_sources_and_a_stale_library_is_refused(tmp_path):
    """The loaded library carries the digest of the sources it was built from (Makefile -> d3f_source_digest); a library
    sitting next to sources it was NOT built from must not load silently."""
    import shutil
    import subprocess
    import sys
    from pathlib import Path
    assert _lib.built_digest() == _lib.source_digest()
    # a copy of the package tree with the built library and one kernel source touched afterwards
    root = Path(_lib.__file__).resolve().parent.parent
    pkg = tmp_path / "denoising_diffusion_deep_fake_amd"
    shutil.copytree(root / "denoising_diffusion_deep_fake_amd", pkg,
                    ignore=shutil.ignore_patterns("build", "__pycache__", "*.o"))
    shutil.copytree(root / "include", tmp_path / "include")
    with open(pkg / "csrc" / "optim.hip", "a") as f:
        f.write("\n// edited after the build\n")
    code = ("from denoising_diffusion_deep_fake_amd import _lib\n"
            "try:\n    _lib.lib()\nexcept _lib.D3FError as e:\n    print('REFUSED', e)\nelse:\n    print('LOADED')\n")
    env = {k: v for k, v in __import__("os").environ.items() if k != "D3F_LIB"}
    out = subprocess.run([sys.executable, "-c", code], cwd=tmp_path, env=env, capture_output=True, text=True)
    assert "REFUSED" in out.stdout and "built from other sources" in out.stdout, (out.stdout, out.stderr)
    # ... while naming the same file explicitly as a variant build loads it
    env["D3F_LIB"] = str(pkg / "csrc" / "libd3f_hip.so")
    out = subprocess.run([sys.executable, "-c", code], cwd=tmp_path, env=env, capture_output=True, text=True)
    assert "LOADED" in out.stdout, (out.stdout, out.stderr)


def test_plan_counts_at_the_headline_shapes():
    """d3f_unet_plan_counts: which kernel family the plan chose for every launch of a training step (planning needs no
    GPU).  A shape or dtype that silently falls back to the implicit GEMM would only show as a slower step; this pins the
    plans the round-5 numbers were measured on: fp32 16x256x256 (7 Winograd + 3 patch / stem forward launches, 5 patch
    weight gradients) and bf16 16x256x256 (32 patch-resident forward + 35 data-gradient launches, 6 + 6 patch-kernel
    launches, the bf16 stem, 22 native-bf16 patch weight gradients); other extents keep the implicit GEMM for the wide
    layers."""
    import ctypes as C
    from denoising_diffusion_deep_fake_amd import _lib
    L = _lib.lib()

    def plan(dtype, B, S):
        h = C.c_void_p()
        assert L.d3f_unet_create(b"resnet34", 3, 3, B, S, S, dtype, C.byref(h)) == 0, L.d3f_last_error()
        f, d, w = (C.c_int32 * 16)(), (C.c_int32 * 16)(), (C.c_int32 * 16)()
        assert L.d3f_unet_plan_counts(h, f, d, w) == 0
        L.d3f_unet_destroy(h)
        return list(f), list(d), list(w)

    f, d, w = plan(_lib.F32, 16, 256)
    assert sum(f) == 47 and f[15] == 7 and f[1] == 2 and f[2] == 1 and f[0] == 37       # Winograd x 7, conv_patch x 2, conv_stem
    assert sum(d) == 50 and d[1] == 2 and d[0] == 48
    assert sum(w) == 51 and w[0] == 44 and w[1] + w[2] + w[3] + w[4] == 7 and w[7] == 0  # (class + skip passes count twice)
    f, d, w = plan(_lib.BF16, 16, 256)
    assert f[9:13] == [7, 8, 12, 5] and f[8] == 1 and f[3] == 2 and f[4] == 1 and f[5] == 1 and f[0] == 10 and f[15] == 0
    assert d[9:13] == [8, 9, 13, 5] and d[3] == 1 and d[4] == 2 and d[6] == 1 and d[7] == 1 and d[0] == 10
    assert w[7] == 22 and w[6] == 1 and w[0] == 25 and sum(w) == 48
    # 128-wide input and the authors' 448: the wide layers' extents do not match the patch-resident forms -> implicit GEMM
    for B, S in ((16, 128), (2, 448)):
        f, d, w = plan(_lib.BF16, B, S)
        assert sum(f[9:13]) == 0 and sum(d[9:13]) == 0 and f[8] == 1 and w[7] == 22


def test_plan_counts_and_workspace_of_the_pair_and_f32x3_plans():
    """The pair plan (two networks, planned together: nets 2, plan_nets 2) at 8x256x256 in fp32 and bf16, and the f32x3
    single-network plan at 16x256x256: every kernel choice (d3f_unet_plan_counts) and the workspace layout's size and
    per-network stride, as recorded before the engine and the C API shared one convolution-layer planner."""
    L = _lib.lib()

    def plan(dtype, B, nets):
        h = C.c_void_p()
        assert L.d3f_unet_create_nets(b"resnet34", 3, 3, B, 256, 256, dtype, nets, nets, C.byref(h)) == 0, L.d3f_last_error()
        f, d, w = (C.c_int32 * 16)(), (C.c_int32 * 16)(), (C.c_int32 * 16)()
        try:
            assert L.d3f_unet_plan_counts(h, f, d, w) == 0
            return list(f), list(d), list(w), L.d3f_unet_workspace_bytes(h), L.d3f_unet_net_workspace_stride(h)
        finally:
            L.d3f_unet_destroy(h)

    assert plan(_lib.F32, 8, 2) == ([37, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7],
                                    [48, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                                    [44, 1, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], 3_620_552_704, 1_810_276_352)
    assert plan(_lib.BF16, 8, 2) == ([10, 0, 0, 2, 1, 1, 0, 0, 1, 7, 8, 12, 5, 0, 0, 0],
                                     [10, 0, 0, 1, 2, 0, 1, 1, 0, 8, 9, 13, 5, 0, 0, 0],
                                     [25, 0, 0, 0, 0, 0, 1, 22, 0, 0, 0, 0, 0, 0, 0, 0], 2_090_164_224, 1_045_082_112)
    assert plan(_lib.F32X3, 16, 1) == ([47, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                                       [50, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                                       [44, 1, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], 3_479_396_608, 0)


def _bn_plan(**kw):
    """d3f_bn_layer_plan of a description (host only); None when the description is refused"""
    L = _lib.lib()
    f = dict(dtype=_lib.F32, C=64, Cpad=None, rows=1000, apply=1, relu=1, res=0, mask=0, fwd_rows=8, fused_rows=0,
             allow_fused=1, plan_nets=1)
    f.update(kw)
    if f["Cpad"] is None:
        f["Cpad"] = f["C"]
    d = _lib.BnDesc(*[f[n] for n, _ in _lib.BnDesc._fields_])
    p = _lib.BnPlan()
    return p if L.d3f_bn_layer_plan(C.byref(d), C.byref(p)) == 0 else None


def test_bn_layer_plan_picks_the_fused_form_inside_its_limits_only():
    """fused only with allow_fused, fp32 / bf16 storage, whole 32-channel slabs and 1..1024 partial rows -- each
    boundary from both sides, forward (fwd_rows) and backward (fused_rows, else the reduce's own rows)"""
    for dtype in (_lib.F32, _lib.BF16):
        for rows_in, want in ((0, False), (1, True), (2, True), (1023, True), (1024, True), (1025, False)):
            p = _bn_plan(dtype=dtype, fwd_rows=rows_in, fused_rows=rows_in, rows=4096)
            assert bool(p.fwd_fused) == want, (dtype, rows_in)
            # (fused_rows = 0: the backward reads bn_bwd_reduce's rows, 1..1024 of them: fused)
            assert bool(p.bwd_fused) == (want or rows_in == 0) and p.bwd_rows == (rows_in or p.reduce_blocks)
        for Cn, want in ((16, False), (32, True), (48, False), (64, True), (96, True), (100, False)):
            p = _bn_plan(dtype=dtype, C=Cn)
            assert (bool(p.fwd_fused), bool(p.bwd_fused)) == (want, want), (dtype, Cn)
            assert (p.rows_per_block > 0) == want
        p = _bn_plan(dtype=dtype, allow_fused=0)
        assert not p.fwd_fused and not p.bwd_fused and p.rows_per_block == 0
        p = _bn_plan(dtype=dtype, apply=0)  # a downsample branch has no streaming pass to fold the finalize into
        assert not p.fwd_fused and p.bwd_fused
    # refused descriptions
    for bad in (dict(C=0), dict(C=64, Cpad=32), dict(rows=-1), dict(res=3), dict(mask=-1), dict(plan_nets=3),
                dict(dtype=7), dict(fwd_rows=-1), dict(fused_rows=-2)):
        assert _bn_plan(**bad) is None, bad
        assert b"bn_layer" in _lib.lib().d3f_last_error()


def test_bn_layer_plan_sizes_cover_what_the_kernels_index():
    """rows_per_block: whole passes of 32 rows, ~256 (fp32) / ~512 (bf16) workgroups in all, half of that per network for
    plan_nets = 2; reduce_blocks in 1..1024; the scratch sizes reach the largest index the kernels read
    (statistics: ((fwd_rows - 1) * Cpad + C - 1) * 2 + 1, partial sums: ((rows - 1) * C + C - 1) * 2 + 1 for the rows
    the reduce writes and for the rows a producer hands in); d3f_bn_backward_workspace_bytes holds the split plan's
    partial rows, three k rows and its alignment slack"""
    L = _lib.lib()
    for dtype, target in ((_lib.F32, 256), (_lib.BF16, 512)):
        for Cn in (32, 64, 128, 512):
            for rows in (1, 2, 31, 32, 33, 1000, 4097, 65536, 262144, 1048576):
                for nets in (1, 2):
                    for fused_rows in (0, 7, 1024, 4096):
                        p = _bn_plan(dtype=dtype, C=Cn, Cpad=Cn + 16, rows=rows, fwd_rows=9, fused_rows=fused_rows,
                                     plan_nets=nets)
                        slabs, T = Cn // 32, target // nets
                        rb = max(1, T // slabs)
                        assert p.rows_per_block % 32 == 0 and p.rows_per_block >= 32
                        blocks = -(-rows // p.rows_per_block)
                        assert blocks * slabs <= max(T, slabs), (dtype, Cn, rows, nets)
                        if rows >= 64 * rb:  # (whole passes of 32 rows cost at most a third of the workgroups then)
                            assert blocks * slabs >= T // 2, (dtype, Cn, rows, nets, blocks)
                        assert 1 <= p.reduce_blocks <= 1024
                        assert p.bwd_rows == (fused_rows or p.reduce_blocks)
                        assert p.stat_floats == 9 * (Cn + 16) * 2 > (8 * (Cn + 16) + Cn - 1) * 2 + 1
                        assert p.part_floats > ((max(p.reduce_blocks, fused_rows) - 1) * Cn + Cn - 1) * 2 + 1
                split = _bn_plan(dtype=dtype, C=Cn, rows=rows, allow_fused=0)
                assert L.d3f_bn_backward_workspace_bytes(dtype, Cn, rows) == \
                    (split.reduce_blocks * Cn * 2 + 3 * Cn) * 4 + 256 >= split.part_floats * 4 + 3 * Cn * 4
    one, two = _bn_plan(rows=65536, plan_nets=1), _bn_plan(rows=65536, plan_nets=2)
    assert two.rows_per_block == 2 * one.rows_per_block and two.reduce_blocks == one.reduce_blocks


def test_bn_layers_of_the_headline_plan():
    """d3f_unet_bn_layer: the description and plan the engine holds for every BatchNorm layer (host only).  The headline
    plan (16 x 256 x 256 fp32, DESIGN.md "BatchNorm (train mode)"): 46 layers; 41 run the fused forward -- all but the
    three downsample branches (apply = 0: only finalized) and the two 16-channel layers of decoder block 4; 44 the fused
    backward (all but decoder block 4), 39 of them on partial rows their producing data gradient wrote; the stem's 1024
    statistics rows are the most the fused form takes.  The same description through d3f_bn_layer_plan gives the same plan."""
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.d3f_unet_create(b"resnet34", 3, 3, 16, 256, 256, _lib.F32, C.byref(h)))
    try:
        assert L.d3f_unet_num_bn(h) == 46
        layers = []
        for i in range(46):
            d, p, q = _lib.BnDesc(), _lib.BnPlan(), _lib.BnPlan()
            _lib.check(L.d3f_unet_bn_layer(h, i, C.byref(d), C.byref(p)))
            _lib.check(L.d3f_bn_layer_plan(C.byref(d), C.byref(q)))
            assert bytes(p) == bytes(q), i
            c = C.c_int()
            rm, rv = C.c_int64(), C.c_int64()
            _lib.check(L.d3f_unet_bn_info(h, i, None, 0, C.byref(c), C.byref(rm), C.byref(rv)))
            assert c.value == d.C and d.dtype == _lib.F32 and d.allow_fused == 1 and d.plan_nets == 1
            layers.append((d, p))
        d = _lib.BnDesc()
        assert L.d3f_unet_bn_layer(h, 46, C.byref(d), C.byref(p)) != 0 and L.d3f_unet_bn_layer(h, -1, C.byref(d), C.byref(p)) != 0
    finally:
        L.d3f_unet_destroy(h)
    assert sum(p.fwd_fused for _, p in layers) == 41
    assert sum(p.bwd_fused for _, p in layers) == 44
    assert sum(d.fused_rows > 0 for d, _ in layers) == 39
    split_fwd = [i for i, (_, p) in enumerate(layers) if not p.fwd_fused]
    assert [layers[i][0].apply for i in split_fwd] == [0, 0, 0, 1, 1]
    assert [layers[i][0].C for i in split_fwd] == [128, 256, 512, 16, 16]
    assert [i for i, (_, p) in enumerate(layers) if not p.bwd_fused] == [44, 45]
    stem_d, stem_p = layers[0]
    assert (stem_d.C, stem_d.rows, stem_d.fwd_rows, stem_d.mask, stem_d.res) == (64, 16 * 128 * 128, 1024, 1, 0)
    assert stem_p.fwd_fused and stem_p.bwd_fused and stem_p.rows_per_block == 2048
    # residual / mask: 16 BasicBlocks end in a residual add (13 identity, 3 downsample branches), masks follow
    assert sum(d.res == 1 for d, _ in layers) == 13 and sum(d.res == 2 for d, _ in layers) == 3
    assert all(d.mask == (0 if not d.apply else 2 if d.res else 1) for d, _ in layers)
