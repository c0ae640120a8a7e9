"""Where the device RNG's streams live (`device_rng: true`, csrc/philox.h).

A draw is a pure function of (seed, offset, image, element).  `seed` is the run's, `offset` names one consumer of one
optimiser step on one rank:

    offset = global_step << 24 | rank << 8 | stream         stream 0: the denoiser / domain a, 1: domain b

The noise, the per-image y and the augmentation uniforms of one (step, rank, stream) never collide: they sit at different
counter groups g of the same offset (normals below 0xFFFFFFFD, the rest above).

Held-out validation (helpers/validation.py) has streams of its own, which never meet a training step's: the step field
holds the position k of the noise ratio in `val_noise_ratios`, the rank is 0 and the stream is 2 (the denoiser / domain a)
or 3 (domain b),

    offset = k << 24 | stream                               stream 2: held-out list / domain a, 3: domain b

and the counter's image word is the image's index in the held-out dataset instead of its place in the batch
(ops.noise_blend_fixed_index_rng): an image meets the same noise every epoch, at any batch size.
"""
MAX_STEP, MAX_RANK, MAX_STREAM = 1 << 40, 1 << 16, 1 << 8


def pack_offset(global_step, rank=0, stream=0):
    global_step, rank, stream = int(global_step), int(rank), int(stream)
    if not 0 <= global_step < MAX_STEP:
        raise ValueError(f"device RNG: global_step {global_step} outside [0, 2**40)")
    if not 0 <= rank < MAX_RANK:
        raise ValueError(f"device RNG: rank {rank} outside [0, 65536)")
    if not 0 <= stream < MAX_STREAM:
        raise ValueError(f"device RNG: stream {stream} outside [0, 256)")
    return global_step << 24 | rank << 8 | stream


def module_stream(module, stream=0, step=None):
    """(seed, offset) of a LightningModule's draws at its current step: seed = hparam `rng_seed` if given, else the trainer's
    rank-independent base seed (saved in checkpoints as d3f_loader_seed, so a resumed run continues the interrupted one),
    else 0 without a trainer; step = `global_step` unless given; rank = the trainer's `global_rank`."""
    trainer = module.trainer
    seed = module.hparams.get("rng_seed")
    if seed is None:
        seed = getattr(trainer, "_base_seed", None) if trainer is not None else None
    rank = getattr(trainer, "global_rank", 0) if trainer is not None else 0
    step = module.global_step if step is None else step
    return int(seed or 0) & 0xFFFFFFFFFFFFFFFF, pack_offset(step, rank, stream)


def refuse_graph_step(hparams):
    if hparams.get("device_rng", False) and hparams.get("graph_step", False):
        raise ValueError("device_rng: true cannot be combined with graph_step: true: the captured whole-step entry "
                         "(d3f_unet_train_step) takes its draws from the caller")
