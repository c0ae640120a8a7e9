/* libd3f_hip.so -- C ABI of the MI355X-native U-Net hot path of d3f
 * (ChainBreak/denoising_diffusion_deep_fake).
 *
 * The reference is pure Python on PyTorch: its "FFI" for this path is the torch op
 * dispatch under `segmentation_models_pytorch.Unet(...)`, `MseStructuralSimilarityLoss`,
 * `torch.optim.Adam` and `ema_pytorch.EMA`.  Each entry point below names the reference
 * call site (file:line under /root/reference) whose device work it replaces.  The Python
 * binding a maintainer adds is a ctypes stub: see INTEGRATION.md and
 * denoising_diffusion_deep_fake_amd/_lib.py.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; d3f_last_error() gives the
 *     thread-local message.
 *   - all pointers are DEVICE pointers borrowed for the duration of the call (memory is
 *     owned by the caller, i.e. PyTorch's allocator); nothing is allocated or freed on the
 *     device by this library.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *     Calls only enqueue work; they never synchronise.
 *   - dtype: 0 = f32, 1 = bf16 (activations / packed weights; master params are f32).
 *   - network boundary tensors are NCHW f32 (what the reference's callers hold);
 *     internal activations are NHWC with channels padded to a 16-byte multiple.
 */
#ifndef D3F_HIP_H
#define D3F_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D3F_F32 0
#define D3F_BF16 1
/* fp32 tensors and fp32 accumulation; the contraction kernels split every fp32 operand exactly into three bf16
 * terms and form each product from six bf16 MFMAs (dropped terms <= 2^-24 |a*b|): fp32-grade results at 6/16 of
 * the fp32 MFMA time.  Everything that is not a contraction is identical to D3F_F32. */
#define D3F_F32X3 2

int d3f_version(void);
const char* d3f_last_error(void);
/* First 16 hex digits of the sha256 over the sources this library was built from (the .hip and .h files of csrc/ and this header; the
 * Makefile bakes it in).  The Python binding refuses a library whose digest differs from the sources next to it
 * (_lib.lib(); D3F_LIB=<path> loads a variant build on purpose and skips the check); bench.py prints it in `config`. */
const char* d3f_source_digest(void);

/* Measurement hooks: when enabled, every launch of the three contraction kernels
 * (class 0 = conv forward, 1 = conv data-gradient, 2 = conv weight-gradient) is bracketed by a pair
 * of HIP events on the launch stream.  collect() waits for them and returns, per class, the summed
 * kernel time (ms), the number of launches and their algorithmic FLOPs, then resets the buffer.
 * max_launches <= 0 disables.  collect() returns 1 if the buffer overflowed.
 * d3f_profile_classes(mask) restricts the bracketing to the classes whose bit is set (default 7 = all):
 * an event pair costs a few microseconds of stream time, so a timed run brackets only what it reports. */
int d3f_profile_enable(int max_launches);
int d3f_profile_classes(int mask);
int d3f_profile_collect(double ms[3], int64_t launches[3], double flops[3]);

/* ---------------------------------------------------------------------------------------
 * Whole-network handle: Unet(encoder_name, encoder_weights=None, in_channels, classes,
 * activation=None) for a fixed (B, H, W, dtype).
 * Replaces: model construction  d3f/train_denoiser/lit_module.py:41-53,
 *                               d3f/train_deep_fake/lit_module.py:49-60
 *           forward             d3f/train_denoiser/lit_module.py:117 (self.model(image_noisy)),
 *                               d3f/train_deep_fake/lit_module.py:173,189,195,266
 *           backward            Lightning's loss.backward() on that module
 * ------------------------------------------------------------------------------------- */
typedef struct d3f_unet* d3f_unet_t;

int d3f_unet_create(const char* encoder_name, int in_channels, int classes, int B, int H, int W,
                    int dtype, d3f_unet_t* out);
int d3f_unet_destroy(d3f_unet_t h);

/* ---------------------------------------------------------------------------------------
 * Two networks, one set of launches.
 * Replaces: the two optimizer steps of one train_deep_fake batch in `mode: "denoise"` --
 *           training_step(batch, batch_idx, optimizer_idx = 0 | 1) -> training_denoise_step_for_one_model("a", batch_a,
 *           model_a) / ("b", batch_b, model_b), d3f/train_deep_fake/lit_module.py:142-181 -- whose forward and backward
 *           passes are INDEPENDENT (model_a never sees domain b) and identical in shape, 8 images each: half of what
 *           fills an MI355X.  A pair handle runs both networks' layer k as ONE kernel launch (gridDim.z carries the
 *           network; a workgroup of network 1 adds byte offsets to its pointers), so every launch has the occupancy of a
 *           16-image batch.  Results are bit for bit those of a single handle created with plan_nets = 2 and run net by
 *           net; swap mode (coupled through the EMA teachers, :183-206) stays sequential.
 * d3f_unet_create_nets: nets = 1 | 2 networks per launch, B images PER network; plan_nets (>= nets): the tile / split-K /
 *           slab / patch-kernel choices count the workgroups of plan_nets networks (nets = 1, plan_nets = 2: the pair's
 *           kernels on one network -- the reference run of the bit-identity test).  d3f_unet_create == (1, 1).
 * Workspace of a pair: ONE buffer of d3f_unet_workspace_bytes(h) bytes = two copies of the single-network layout,
 *           d3f_unet_net_workspace_stride(h) bytes apart (d3f_unet_export on network 1: pass workspace + stride).
 * The pair entry points take the two networks' buffers as arrays of two pointers (any two allocations); train-mode
 *           forward only, per-GPU BatchNorm statistics only.  Packing, forward and backward of a pair handle go through
 *           these three calls; everything per network (noise blend, loss, Adam, EMA) stays the single-network entry
 *           points, called once per network.  On a pair handle d3f_unet_pack_weights, _forward, _forward_graph,
 *           _predict_u8, _backward, _backward_nojoin, _train_step and d3f_unet_set_bn_sync with a callback (fn != NULL)
 *           return an error before anything is enqueued; the queries, d3f_unet_set_bn_sync(h, NULL, ...), the side
 *           stream, d3f_unet_backward_join and d3f_unet_export / _export_shape take either kind of handle.
 * ------------------------------------------------------------------------------------- */
int d3f_unet_create_nets(const char* encoder_name, int in_channels, int classes, int B, int H, int W, int dtype,
                         int nets, int plan_nets, d3f_unet_t* out);
int d3f_unet_nets(d3f_unet_t h);
size_t d3f_unet_net_workspace_stride(d3f_unet_t h);
int d3f_unet_pair_pack_weights(d3f_unet_t h, const float* const params[2], void* workspace, void* stream);
int d3f_unet_pair_forward(d3f_unet_t h, const float* const params[2], float* const bnstats[2], const float* const x[2],
                          float* const out[2], void* workspace, void* stream);
/* join != 0: every gradient of the segments is final on `stream` on return (d3f_unet_backward); join == 0: the
 * d3f_unet_backward_nojoin contract (final on the engine's side stream; d3f_unet_backward_join later) */
int d3f_unet_pair_backward(d3f_unet_t h, const float* const params[2], const float* const grad_out[2],
                           float* const grads[2], void* workspace, int seg_begin, int seg_end, int join, void* stream);

/* The `activation` argument of Unet(...): smp's Activation module, which smp.Unet applies last in its SegmentationHead
 * (the model the reference builds at d3f/train_denoiser/lit_module.py:46-52 with activation=None), over the head's
 * convolution output z [B][classes][H][W]:
 *   D3F_ACT_IDENTITY    z                                            (None, "identity")
 *   D3F_ACT_SIGMOID     1 / (1 + exp(-z))
 *   D3F_ACT_TANH        tanh(z)
 *   D3F_ACT_SOFTMAX     softmax over the channel axis per pixel      ("softmax2d", and "softmax": nn.Softmax() without
 *                       dim resolves to dim = 1 for a 4-D input)
 *   D3F_ACT_LOGSOFTMAX  log-softmax over the channel axis
 *   D3F_ACT_CLAMP       clamp(z, 0, 1)                               (smp's default bounds)
 * in fp32 whatever the compute dtype.  Host only, either kind of handle (a pair's two networks share the setting); the
 * default after d3f_unet_create / d3f_unet_create_nets is identity, whose launches are exactly those of a handle that
 * never heard of activations.  Every entry point honours the setting: d3f_unet_forward (both modes), _forward_graph,
 * _pair_forward, _predict_u8 and _predict_frames_u8 (applied inside their last kernel), _backward, _backward_nojoin,
 * _pair_backward (the upstream gradient is the one w.r.t. the ACTIVATED output; z is kept in the workspace by the
 * training forward, so the caller may overwrite `out` before backward; segment 0 of the backward pass turns z into dz in
 * place, so an activated head takes ONE backward pass per training forward: a second one is an error, not a wrong
 * gradient) and _train_step.  The workspace size does not depend on the setting.  Setting a different value
 * drops the handle's captured graphs (eval, predict, frames, step), as a pointer change does.  argmax heads return
 * integer tensors without a gradient and are not offered. */
#define D3F_ACT_IDENTITY 0
#define D3F_ACT_SIGMOID 1
#define D3F_ACT_TANH 2
#define D3F_ACT_SOFTMAX 3
#define D3F_ACT_LOGSOFTMAX 4
#define D3F_ACT_CLAMP 5
int d3f_unet_set_head_activation(d3f_unet_t h, int act);
int d3f_unet_head_activation(d3f_unet_t h); /* the code, or < 0 for a null handle */

/* parameter table, in torch named_parameters() order; offsets are in floats into ONE flat
 * f32 buffer that holds every parameter (gradients use the same layout). */
int d3f_unet_num_params(d3f_unet_t h);
int d3f_unet_param_info(d3f_unet_t h, int i, char* name, int name_cap, int32_t shape[4], int* ndim,
                        int64_t* offset);
int64_t d3f_unet_param_floats(d3f_unet_t h);
/* BatchNorm running statistics: flat f32 buffer, per layer running_mean[C] then running_var[C] */
int d3f_unet_num_bn(d3f_unet_t h);
int d3f_unet_bn_info(d3f_unet_t h, int i, char* prefix, int prefix_cap, int* C, int64_t* rm_offset,
                     int64_t* rv_offset);
int64_t d3f_unet_bnstat_floats(d3f_unet_t h);
size_t d3f_unet_workspace_bytes(d3f_unet_t h);
/* algorithmic conv FLOPs (2*MAC, unpadded channels) of one forward / one backward call */
double d3f_unet_forward_flops(d3f_unet_t h);
double d3f_unet_backward_flops(d3f_unet_t h);

/* re-pack the f32 master weights into the kernels' layouts (call after every parameter update) */
int d3f_unet_pack_weights(d3f_unet_t h, const float* params, void* workspace, void* stream);
/* x, out: NCHW f32 [B][in_channels|classes][H][W].  training != 0: BatchNorm uses batch statistics,
 * updates bnstats (momentum 0.1) and keeps what backward needs in the workspace. */
int d3f_unet_forward(d3f_unet_t h, const float* params, float* bnstats, const float* x, float* out,
                     void* workspace, int training, void* stream);
/* The eval-mode forward (training == 0 above: BatchNorm running statistics folded into the conv epilogues) replayed
 * from a hipGraph that is captured on first use per set of pointers (params, bnstats, x, out, workspace) -- the
 * "hipGraph-captured denoise step" of BASELINE.json configs[4]; the reference's frame loop is
 * d3f/script_tools/put_video_through_fake_model.py:111-119 -> d3f/train_deep_fake/lit_module.py:259-270.  Results are
 * bit-identical to d3f_unet_forward(training = 0); parameter VALUES are read at replay time (only pointers are baked
 * in), so the graph survives optimiser / EMA updates followed by d3f_unet_pack_weights. */
int d3f_unet_forward_graph(d3f_unet_t h, const float* params, float* bnstats, const float* x, float* out,
                           void* workspace, void* stream);
/* Inference entry behind LitModule.predict_fake_for_single_frame (d3f/train_deep_fake/lit_module.py:259-300):
 * uint8 BGR frames [B][H][W][3] in device memory -> eval-mode forward (BatchNorm folded into the conv
 * epilogues) -> uint8 BGR frames, with cv2_to_tensor_normalised (:272-283: BGR->RGB, (x - mean*255) / (std*255))
 * and tensor_cv2_to_denormalised (:285-300: x*std*255 + mean*255, .int() truncation, clamp 0..255, RGB->BGR)
 * fused into the first and last kernel.  mean / std: 3 host floats (RGB order).  use_graph != 0: the launch
 * sequence is captured into a hipGraph on first use (per set of pointers) and replayed afterwards. */
int d3f_unet_predict_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* bgr_in, uint8_t* bgr_out,
                        const float mean[3], const float std[3], void* workspace, int use_graph, void* stream);
/* The frame loop of d3f/script_tools/put_video_through_fake_model.py:54-70, 111-145 on decoded frames of any size:
 * raw_in [B][src_h][src_w][3] uint8 BGR in device memory -> crop box (x1, y1, cw, ch) -> bicubic resize to the handle's
 * H x W (d3f_crop_resize_cubic_u8 below) -> d3f_unet_predict_u8 -> pair_out [B][H][2W][3]: the left half is the resized
 * real frame, the right half the fake (np.concatenate([real, fake], axis=1)).  Three steps around the forward pass:
 * one kernel writes the real half and, from the same rounded bytes, the normalised network input (the reference
 * normalises cv2's uint8 result); the last kernel writes the fake half.  The left half is byte for byte
 * d3f_crop_resize_cubic_u8, the right half d3f_unet_predict_u8 of the left half.  The crop box is the caller's
 * (crop_image_at_center's float arithmetic stays in Python: ops.center_crop_box).  use_graph != 0: captured on first use
 * per set of pointers, frame size, crop box and mean / std, replayed afterwards.  Per-frame results do not depend on the
 * other frames of a batch, but the plan's kernel choices depend on B: bytes are not promised equal across batch sizes. */
int d3f_unet_predict_frames_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in, int src_h,
                               int src_w, int x1, int y1, int cw, int ch, uint8_t* pair_out, const float mean[3],
                               const float std[3], void* workspace, int use_graph, void* stream);
/* The swapped video at the source's size (nothing in the reference: its tool stops at the real|fake pair).  Exactly the
 * launches of d3f_unet_predict_frames_u8 into pair_out [B][H][2W][3], then ONE d3f_paste_resize_cubic_u8 launch (below):
 * patch = the right half of pair_out (row stride 6 * W), frame = raw_in, out = full_out [B][src_h][src_w][3], same box.
 * pair_out holds the bytes d3f_unet_predict_frames_u8 writes, full_out the bytes d3f_paste_resize_cubic_u8 gives on them,
 * both bit for bit; the caller owns both buffers (pair_out doubles as the fake's staging buffer; nothing is allocated).
 * full_out == raw_in pastes in place and is refused together with use_graph: a replay would read frames it has already
 * overwritten.  use_graph != 0: captured on first use per set of pointers (full_out included), frame size, crop box,
 * feather and mean / std, in a graph slot of its own (alternating with d3f_unet_predict_frames_u8 re-captures neither).
 * Refused as d3f_unet_predict_frames_u8 refuses: a pair handle, a null argument, a network that is not 3 -> 3 channels;
 * and whatever either operator refuses, before any capture. */
int d3f_unet_predict_frames_full_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in, int src_h,
                                    int src_w, int x1, int y1, int cw, int ch, int feather, uint8_t* pair_out,
                                    uint8_t* full_out, const float mean[3], const float std[3], void* workspace,
                                    int use_graph, void* stream);
/* The two frame entries with a box per frame (a face that moves through the frames): the signatures above with boxes in
 * place of x1, y1, cw, ch -- HOST memory, [B][4] int32 as x1, y1, cw, ch of frame b, B the handle's batch size, read before
 * the call returns.  The same launch sequence with the crop and the paste in their boxes forms
 * (d3f_crop_resize_cubic_boxes_u8 / _aa_boxes_u8, d3f_paste_resize_cubic_boxes_u8 / _color_boxes_u8 below): pair_out and
 * full_out are byte for byte the composition of those operators, as the single-box entries are of theirs, and every frame
 * setting (resample, colour match, temporal filter) applies unchanged -- they work on pair_out, where a box is no longer
 * seen.  (The temporal filter's gate reads the resized real crop: a box that moves is motion to it.)  One feather for the
 * call.  use_graph != 0 is REFUSED: a captured launch bakes its kernel arguments in, the boxes among them, and a graph keyed
 * on their values would be re-captured on every call of a moving box; replay needs the boxes in device memory, which these
 * entries do not have.  Refused before any device call besides: what the single-box entries refuse, a null boxes, and for
 * any frame what the boxes operators refuse of its box, with the frame's index in the message. */
int d3f_unet_predict_frames_boxes_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in, int src_h,
                                     int src_w, const int32_t* boxes, uint8_t* pair_out, const float mean[3],
                                     const float std[3], void* workspace, int use_graph, void* stream);
int d3f_unet_predict_frames_full_boxes_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in,
                                          int src_h, int src_w, const int32_t* boxes, int feather, uint8_t* pair_out,
                                          uint8_t* full_out, const float mean[3], const float std[3], void* workspace,
                                          int use_graph, void* stream);
/* The two boxes entries with a rotation per frame (a head that rolls): rot is HOST memory, [B][2] int32 as c16, s16 of frame
 * b (the _rboxes_ operators below define them), read before the call returns.  The same launch sequence with the crop and the
 * paste in their rotated forms (d3f_crop_resize_cubic_rboxes_u8_nhwc, d3f_paste_resize_cubic_rboxes_u8 / _color_rboxes_u8):
 * pair_out and full_out are byte for byte the composition of those operators; colour sums, coefficients, their smoothing and
 * the temporal filter work on pair_out and do not change.  Refused before any device call: what the boxes entries refuse
 * (use_graph != 0 among it, for their reason), a null rot, a rot that is no rotation (the frame is named), and
 * D3F_RESAMPLE_CUBIC_AA or D3F_BLEND_MULTIBAND on the handle -- the antialiased crop and the multiband pyramid of a rotated
 * box are out of scope. */
int d3f_unet_predict_frames_rboxes_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in, int src_h,
                                      int src_w, const int32_t* boxes, const int32_t* rot, uint8_t* pair_out,
                                      const float mean[3], const float std[3], void* workspace, int use_graph, void* stream);
int d3f_unet_predict_frames_full_rboxes_u8(d3f_unet_t h, const float* params, float* bnstats, const uint8_t* raw_in,
                                           int src_h, int src_w, const int32_t* boxes, const int32_t* rot, int feather,
                                           uint8_t* pair_out, uint8_t* full_out, const float mean[3], const float std[3],
                                           void* workspace, int use_graph, void* stream);
/* How d3f_unet_predict_frames_u8 and d3f_unet_predict_frames_full_u8 resize the crop box to the handle's H x W:
 *   D3F_RESAMPLE_CUBIC     d3f_crop_resize_cubic_u8 (cv2.INTER_CUBIC: four taps per axis whatever the scale).  The default
 *                          after d3f_unet_create; its launches are exactly those of a handle that never heard of the setting.
 *   D3F_RESAMPLE_CUBIC_AA  d3f_crop_resize_cubic_aa_u8 (Pillow's antialiased bicubic: the window widens with the scale).
 * The crop-to-network step only: the paste of the full-frame entry enlarges and stays d3f_paste_resize_cubic_u8.  With
 * D3F_RESAMPLE_CUBIC_AA the left half of pair_out is byte for byte d3f_crop_resize_cubic_aa_u8 (one kernel writes it and,
 * from the same rounded bytes, the normalised network input), the right half d3f_unet_predict_u8 of the left half, and
 * the entries refuse what that operator refuses (a crop above 32 times the output on an axis) before any capture.
 * Host only.  Setting a different value drops the handle's captured frames and full-frame graphs, as a pointer change does;
 * an unknown mode and a pair handle (which has no frame entries) are refused. */
#define D3F_RESAMPLE_CUBIC 0
#define D3F_RESAMPLE_CUBIC_AA 1
int d3f_unet_set_frame_resample(d3f_unet_t h, int mode);
int d3f_unet_frame_resample(d3f_unet_t h); /* the mode, or < 0 for a null handle */
/* Whether d3f_unet_predict_frames_full_u8 matches the fake's colour to the resized real crop before it pastes:
 *   D3F_COLOR_NONE     no.  The default after d3f_unet_create; the launches are exactly those of a handle that never heard
 *                      of the setting.
 *   D3F_COLOR_MEANSTD  after the launches into pair_out, TWO more launches and the paste in its colour form: one launch takes
 *                      the sums of d3f_channel_sums_u8 over both halves of pair_out (every workgroup stores a partial row; no
 *                      accumulator to reset), one adds the rows in a fixed order and forms d3f_color_match_coef's
 *                      coefficients with from = the right half (the fake) and to = the left half (the resized real crop),
 *                      n = H * W; then d3f_paste_resize_cubic_color_u8.  full_out is bit for bit the composition of the three
 *                      operators on pair_out; pair_out itself stays byte for byte what d3f_unet_predict_frames_u8 writes.
 * The partial sums and the coefficients live in device memory that belongs to the handle: allocated at the first switch to a
 * mode other than D3F_COLOR_NONE, freed with the handle, nothing inside a frame call.  d3f_unet_predict_frames_u8 ignores the
 * mode.  The mode is part of the full-frame graph's key, and setting a different value drops the handle's captured frames and
 * full-frame graphs.  Refused: an unknown mode, a pair handle, and a handle whose H * W is above 2^22 (at set time). */
#define D3F_COLOR_NONE 0
#define D3F_COLOR_MEANSTD 1
int d3f_unet_set_frame_color_match(d3f_unet_t h, int mode);
int d3f_unet_frame_color_match(d3f_unet_t h); /* the mode, or < 0 for a null handle */
/* The temporal filter of the two frame entries (d3f_temporal_filter_u8, d3f_color_coef_smooth below).  strength == 0 is off and
 * the default after d3f_unet_create: the launches, bytes and graphs are exactly those of a handle that never heard of the
 * setting.  strength in (0, 1), threshold in 1..255:
 *   - d3f_unet_predict_frames_u8 runs its launches, then d3f_temporal_filter_u8 on pair_out (real = the left half, fake = the
 *     right half, both with row stride 6 * W, in place) and the flag launch: the right half of pair_out then holds the
 *     FILTERED fake, bit for bit the operator's on the bytes the plain entry writes;
 *   - d3f_unet_predict_frames_full_u8 does the same and pastes from the filtered half.  With D3F_COLOR_MEANSTD the order is
 *     filter, sums over both halves (the filtered fake), coefficients, d3f_color_coef_smooth with to = the left half's sums
 *     and n = H * W, the colour paste.
 * Every call of either entry advances the handle's time by B frames: the frames of successive calls are consecutive.  The
 * state of both operators lives in device memory of the handle at fixed addresses (a captured graph replays correctly):
 * allocated at the first switch on, freed with the handle, nothing inside a frame call.  The smoothing's state advances only
 * in calls that run it (the full-frame entry with D3F_COLOR_MEANSTD).  Setting the values the handle has changes nothing, not
 * the state and not a captured graph; different values drop the two frame graphs and make the next frame a first frame (the
 * reset is enqueued on that call's stream).  Strength bits and threshold are part of both graph keys.
 * d3f_unet_frame_temporal reads the setting (either pointer may be null); d3f_unet_frame_temporal_reset makes the next frame
 * a first frame by work on `stream`, without dropping graphs (a no-op while the mode has never been on).  Refused: a pair
 * handle, strength outside [0, 1) or NaN, threshold outside 1..255. */
int d3f_unet_set_frame_temporal(d3f_unet_t h, float strength, int threshold);
int d3f_unet_frame_temporal(d3f_unet_t h, float* strength, int* threshold);
int d3f_unet_frame_temporal_reset(d3f_unet_t h, void* stream);
/* How the full-frame entries (d3f_unet_predict_frames_full_u8, _full_boxes_u8) blend the fake into the frame:
 *   D3F_BLEND_FEATHER    one ramp of `feather` pixels: d3f_paste_resize_cubic_u8 (with D3F_COLOR_MEANSTD its colour form).  The
 *                        default after d3f_unet_create; launches, bytes and graphs are exactly those of a handle that never
 *                        heard of the setting, and `levels` is ignored (and kept).
 *   D3F_BLEND_MULTIBAND  the last launch -- the paste -- is replaced by the launches of d3f_paste_multiband_u8 (with
 *                        D3F_COLOR_MEANSTD: sums, coefficients, their smoothing, then d3f_paste_multiband_color_u8; with boxes
 *                        the boxes forms) with levels in 1..D3F_MULTIBAND_MAX_LEVELS: full_out is byte for byte that
 *                        operator on pair_out's fake half.  The temporal filter acts on the pair before the paste and is
 *                        untouched; d3f_unet_predict_frames_u8 ignores the setting.
 * The pyramid workspace belongs to the handle: sized by d3f_paste_multiband_workspace_bytes for the call's batch and largest
 * box, grown (never shrunk) at the start of a full-frame call that needs more, before anything is enqueued or captured, and
 * freed with the handle; a growth waits for the device and drops the full-frame graph.  Mode and levels are part of the
 * full-frame graph's key.  Setting the values the handle has changes nothing; different values drop the two frame graphs.
 * Refused: an unknown mode, levels outside 1..6 with D3F_BLEND_MULTIBAND, a pair handle; at the call, whatever the operator
 * refuses (a box below 1 << levels on a side), before any capture. */
#define D3F_BLEND_FEATHER 0
#define D3F_BLEND_MULTIBAND 1
int d3f_unet_set_frame_blend(d3f_unet_t h, int mode, int levels);
int d3f_unet_frame_blend(d3f_unet_t h, int* levels); /* the mode (levels, if not null, gets the levels), or < 0 for a null handle */
/* gradients of every parameter (written, not accumulated) for the preceding training forward.
 * The backward pass is cut into d3f_unet_num_segments() buckets so a data-parallel caller can
 * all-reduce bucket k while bucket k+1 computes: run segments [seg_begin, seg_end) in order 0..n;
 * after segment k, grads[begin_k, end_k) (floats) are final. */
int d3f_unet_num_segments(d3f_unet_t h);
/* Which kernel family the plan chose for every launch of a training step (a regression guard: falling back to the
 * implicit GEMM is silent otherwise).  fwd / dgrad count launches by ConvParams::patch (0 = conv_igemm_kernel, 1 / 3-7 =
 * conv_patch_kernel forms, 2 / 8 = conv_stem[_bf16]_kernel, 9-12 = conv_pres_kernel for 64 / 128 / 256 / 512 channels;
 * slot 15 of fwd = conv_winograd_kernel), wgrad by WgradParams::patch (0 = tap-parallel conv_wgrad_kernel, 1-6 = the
 * fp32-MFMA patch kernels incl. the stem's, 7 = conv_wgrad_patch_bf16_kernel).  Replaces nothing in the reference: the
 * conv2d dispatches of smp.Unet under d3f/train_denoiser/lit_module.py:117 choose their kernels inside ATen. */
int d3f_unet_plan_counts(d3f_unet_t h, int32_t fwd[16], int32_t dgrad[16], int32_t wgrad[16]);
int d3f_unet_segment_range(d3f_unet_t h, int segment, int64_t* begin, int64_t* end);
int d3f_unet_backward(d3f_unet_t h, const float* params, const float* grad_out, float* grads,
                      void* workspace, int seg_begin, int seg_end, void* stream);
/* Data-parallel form (BASELINE.json: "RCCL all-reduce of gradients over xGMI overlapped with the backward pass";
 * the reference itself is single-device, d3f/train_deep_fake/start_training.py:43-48).  d3f_unet_backward makes the
 * caller's stream -- the critical path of the backward pass -- wait for the engine's weight-gradient stream before it
 * returns; called once per bucket that stalls the chain four times.  d3f_unet_backward_nojoin enqueues the same work
 * and makes NOTHING wait on the caller's stream: the gradients of the segments are final on the engine's side stream
 * (d3f_unet_side_stream; NULL in D3F_SERIAL_BACKWARD mode = the caller's stream) once everything enqueued there so far
 * has run, so a collective ordered behind THAT stream overlaps the remaining segments.  d3f_unet_backward_join makes
 * `stream` wait for the side stream (call once, before the optimiser reads the gradients). */
int d3f_unet_backward_nojoin(d3f_unet_t h, const float* params, const float* grad_out, float* grads,
                             void* workspace, int seg_begin, int seg_end, void* stream);
int d3f_unet_side_stream(d3f_unet_t h, void** stream_out);
int d3f_unet_backward_join(d3f_unet_t h, void* stream);
/* One whole optimiser step of the reference's noisy -> clean objective as ONE call -- what Lightning's automatic
 * optimisation runs around d3f/train_denoiser/lit_module.py:107-126 (and training_denoise_step_for_one_model,
 * d3f/train_deep_fake/lit_module.py:162-181): pack weights -> blend_random_amount_of_noise_with_each_sample (the noise
 * and the uniform draws come from the caller: RNG stays outside) -> forward -> MseStructuralSimilarityLoss -> backward ->
 * Adam.  use_graph != 0: the ~330 kernel launches over the engine's streams are captured into a hipGraph on first use
 * (per set of pointers) and replayed with one launch; results are bit-identical to the separate calls.  Every buffer is
 * the caller's and must stay where it is between calls (pointers are baked into the graph); `adam_coef` is DEVICE memory
 * holding the 8 floats d3f_adam_coefficients() computes on the host for this step (lr, betas, bias corrections), copied
 * there stream-ordered before the call. */
typedef struct d3f_step_buffers {
  float* params; float* bnstats; float* grads; float* exp_avg; float* exp_avg_sq;  /* flat buffers of the network */
  const float* image;      /* [B][3][H][W] clean batch = the loss target */
  const float* noise;      /* randn, same shape */
  const float* y_uniform;  /* rand(B) */
  float* noisy;            /* scratch [B][3][H][W] */
  float* pred;             /* network output [B][3][H][W] */
  float* grad_pred;        /* d loss / d pred */
  float* loss_out;         /* {loss, mse, ssim} */
  void* loss_workspace;    /* d3f_mse_ssim_loss_workspace_bytes(B, H, W) */
  const float* adam_coef;  /* device, 8 floats */
} d3f_step_buffers;
int d3f_adam_coefficients(float lr, float beta1, float beta2, float eps, int step, float grad_scale, float coef[8]);
int d3f_unet_train_step(d3f_unet_t h, const d3f_step_buffers* buffers, float lambda, float input_min, float input_max,
                        void* workspace, int use_graph, void* stream);
/* Optional synchronised BatchNorm (what pytorch_lightning's Trainer(sync_batchnorm=True) would add to the
 * reference's Trainer(gpus=1) at d3f/train_deep_fake/start_training.py:43-48): with a callback installed, every
 * train-mode BatchNorm takes its batch statistics -- and the two sums of its backward pass -- over ALL ranks' batches.
 * fn must sum-all-reduce `count` floats at `data` (a region of the workspace handed to forward / backward) in place,
 * ordered on `stream`, and return 0; it is called from inside d3f_unet_forward / d3f_unet_backward, once per BatchNorm
 * layer each.  fn == NULL: per-GPU statistics (the default).  The fused finalize kernels are bypassed in this mode. */
typedef int (*d3f_allreduce_fn)(void* ctx, float* data, int64_t count, void* stream);
int d3f_unet_set_bn_sync(d3f_unet_t h, d3f_allreduce_fn fn, void* ctx, int world_size);
/* debugging / tests: copy an internal activation ("<conv name>:y" raw conv output, ":a" post
 * BN+ReLU, ":da" its gradient) to NCHW f32 */
int d3f_unet_export(d3f_unet_t h, const char* name, const void* workspace, float* out_nchw, void* stream);
/* extent of that tensor: dims = {channels (as stored: padded to the vector width), height, width} */
int d3f_unet_export_shape(d3f_unet_t h, const char* name, int32_t dims[3]);

/* ---------------------------------------------------------------------------------------
 * Single operators (the kernels the network is made of; used by the parity tests)
 * ------------------------------------------------------------------------------------- */
typedef struct d3f_conv_desc {
  int32_t B, H, W;    /* extent of the conv input (after the optional x2 up-sampling of src0) */
  int32_t C0, C1;     /* channels of src0 and of the concatenated src1 (0: none); padded to 4 (f32) / 8 (bf16) */
  int32_t upsample0;  /* 1: src0 is [B][H/2][W/2][C0], read through nearest x2 up-sampling; 2: the same, and
                       * d3f_conv_backward_data may hand back dx0 at that LOW resolution (see there) */
  int32_t Cout, KH, KW, stride, pad;
  int32_t CinReal;    /* unpadded input channels of the f32 master weight [Cout][CinReal][KH][KW] */
} d3f_conv_desc;

/* torch.nn.Conv2d weight -> packed forward (which=0) / data-gradient (which=1) operand.  d3f_conv_pack_weights packs
 * with the whole-network packing kernel, whose table holds 16-bit extents and 32-bit element indices: a layer whose
 * padded extents (Cout, Cin, their padded row counts, KH*KW*Cin and KH*KW*Cout rounded up to whole k-tiles) reach 65536,
 * or one of whose requested layouts reaches 2^31 elements, is refused with an error naming that limit (an up-sampled
 * layer that runs folded, d3f_conv_upsample_folded, is packed by a kernel of its own, as before).
 * d3f_conv_packed_bytes still sizes such a layer. */
size_t d3f_conv_packed_bytes(int dtype, const d3f_conv_desc* d, int which);
int d3f_conv_pack_weights(int dtype, const d3f_conv_desc* d, const float* w, void* w_fwd, void* w_dgrad,
                          void* stream);
/* y = conv(cat(up(src0), src1)) NHWC; stats != NULL: per-channel (sum, sumsq) partials for
 * d3f_bn_finalize, d3f_conv_stats_floats() floats.  Replaces F.interpolate + torch.cat + conv2d
 * of smp's DecoderBlock / torchvision BasicBlock under lit_module.py:117. */
/* `workspace` (optional, d3f_conv_workspace_bytes(.., which) bytes; which 0 = forward, 1 = data
 * gradient) lets layers whose M x Cout yields too few workgroups split their K loop (split-K slabs
 * + fixed-order reduce); the statistics partial layout then follows the reduce kernel, so pass the
 * same with_workspace flag to d3f_conv_stats_floats. */
size_t d3f_conv_workspace_bytes(int dtype, const d3f_conv_desc* d, int which);
size_t d3f_conv_stats_floats(int dtype, const d3f_conv_desc* d, int with_workspace, int* tiles);
int d3f_conv_forward(int dtype, const d3f_conv_desc* d, const void* src0, const void* src1,
                     const void* w_fwd, void* y, float* stats, void* workspace, void* stream);
/* The Winograd F(2x2, 3x3) form of the same convolution for fp32 layers with a 3x3 / stride 1 / pad 1 kernel, one
 * source, H and W multiples of 16, C0 a multiple of 16 and Cout a multiple of 64 (any other shape: D3F_EINVAL) -- the
 * conv2d of torchvision's BasicBlock under smp.Unet(resnet34), d3f/train_denoiser/lit_module.py:46-52, :117.  The
 * whole-network plan takes it where d3f_conv_winograd_applies() == 1 (at least 256 workgroups of 16x16 pixels x 64
 * filters); this entry runs it on any shape it fits.  u: filters transformed by d3f_conv_winograd_pack from the torch
 * weight [Cout][C0][3][3] (d3f_conv_winograd_filter_bytes bytes).  scale == NULL: y = conv(src0), stats (optional) =
 * one (sum, sumsq) row per workgroup, d3f_conv_winograd_stats_floats() floats for d3f_bn_finalize.  scale != NULL:
 * the eval epilogue y = relu?(conv(src0) * scale[c] + shift[c] + residual?) of the BatchNorm-folded forward. */
int d3f_conv_winograd_applies(int dtype, const d3f_conv_desc* d);
size_t d3f_conv_winograd_filter_bytes(const d3f_conv_desc* d);
size_t d3f_conv_winograd_stats_floats(const d3f_conv_desc* d, int* tiles);
int d3f_conv_winograd_pack(const d3f_conv_desc* d, const float* w, void* u, void* stream);
int d3f_conv_winograd_forward(const d3f_conv_desc* d, const void* src0, const void* u, void* y, float* stats,
                              const float* scale, const float* shift, const void* residual, int relu, void* stream);
/* dx over the conv input: channels [0,C0) -> dx0, [C0,C0+C1) -> dx1; acc*: add to the destination instead of
 * overwriting.  With upsample0, dx0 is the gradient of the LOW-resolution source [B][H/2][W/2][C0] when the layer
 * runs with the up-sampling folded into pre-summed weights (d3f_conv_upsample_folded() == 1: 3x3, stride 1, pad 1,
 * whole k-tiles per tap -- every decoder layer of the network), else the full-resolution [B][H][W][C0] gradient of
 * the up-sampled operand, to be reduced with d3f_upsample2x_backward.  Opt-in third form: a caller that sets
 * upsample0 = 2 in the descriptor AND finds d3f_conv_upsample_summed() == 1 (bf16 storage, 16 -> 32 channels, one source:
 * decoder.blocks.4.conv1 of smp's UnetDecoder, the F.interpolate + conv2d pair under d3f/train_denoiser/lit_module.py:117)
 * gets the 2x2 blocks summed in the launch's epilogue: dx0 is the LOW-resolution gradient as in the folded case.  With
 * upsample0 = 1 that layer keeps the full-resolution contract. */
int d3f_conv_upsample_folded(int dtype, const d3f_conv_desc* d);
int d3f_conv_upsample_summed(int dtype, const d3f_conv_desc* d);
int d3f_conv_backward_data(int dtype, const d3f_conv_desc* d, const void* dy, const void* w_dgrad,
                           void* dx0, void* dx1, int acc0, int acc1, void* workspace, void* stream);
/* dw in torch layout [Cout][CinReal][KH][KW] f32 */
size_t d3f_conv_backward_weight_workspace_bytes(int dtype, const d3f_conv_desc* d);
int d3f_conv_backward_weight(int dtype, const d3f_conv_desc* d, const void* dy, const void* src0,
                             const void* src1, void* workspace, float* dw, void* stream);

/* Plan introspection (host only, nothing is launched): which kernel instantiation each launch of a convolution layer
 * takes, read from the very layer description the three calls above plan -- a regression guard, and the table the operator
 * tests key their cases to.  A launch the layer does not have (or that the description cannot run through the
 * single-operator entry, e.g. a forward with Cout % 4 != 0, a data gradient of a convolution that is neither 'same' nor
 * exactly halving) has planned == 0 and every other field 0. */
typedef struct d3f_conv_launch_plan {
  int32_t planned;
  int32_t patch;             /* ConvParams::patch: 0 = conv_igemm_kernel, 1 / 3-7 conv_patch_kernel forms, 2 / 8 the stem
                              * kernels, 9-12 conv_pres_kernel for 64 / 128 / 256 / 512 channels */
  int32_t tile_bm, tile_bn;  /* conv_igemm_kernel's tile (0 for the patch kernels) */
  int32_t tiles_m, tiles_n, splitk; /* splitk > 1: split-K slabs + conv_splitk_reduce_kernel */
  int32_t par, nz;           /* output-parity form (1 / 2 stride-2 data gradient, 3 up-folded forward), classes per launch */
  int32_t small_c;           /* conv_igemm_kernel's small-channel loader (a k-row spans taps) */
  int32_t fast_addr;         /* its plain-gather loader, as the launch decides it (both 0 for the patch kernels) */
  int32_t sum2;              /* data gradient stored 2x2-summed at half resolution */
  int32_t stat_rows;         /* forward: statistics rows written ([stat_rows][CoutPad][2]) */
} d3f_conv_launch_plan;
typedef struct d3f_conv_wgrad_plan {
  int32_t part, cls;         /* 0 whole layer, 1 class form of the up-sampled source, 2 the skip tensor; cls: 16 folded taps */
  int32_t patch;             /* 0 tap-parallel conv_wgrad_kernel, 1-3 persistent patch kernel, 4 / 5 / 6 the stem's, 7 native bf16 */
  int32_t splits;            /* slabs = workgroup columns */
  int32_t chunks_per_split;  /* tap-parallel: 32-pixel chunks per slab (the last slab takes the rest); persistent: 0 */
  int32_t tile;              /* tap-parallel: 32 or 64 (co x ci tile edge); persistent: 0 */
  int32_t tiles;             /* tap-parallel: chunks in all; persistent: spatial tiles the `splits` workgroups stride over */
} d3f_conv_wgrad_plan;
typedef struct d3f_conv_plan {
  int32_t upfold;            /* up-sampling folded into pre-summed weights (forward par 3, dgrad_lo + dgrad of the skip tensor) */
  int32_t parity;            /* stride-2 data gradient as output-parity classes */
  int32_t wino, wino_rows;   /* the whole-network plan runs the forward as Winograd; its statistics rows where the kernel fits */
  d3f_conv_launch_plan fwd, dgrad, dgrad_lo; /* dgrad_lo: the up-folded layer's low-resolution source (then dgrad: its skip tensor) */
  int32_t wgrad_parts;       /* 1 or 2 */
  d3f_conv_wgrad_plan wgrad[2];
} d3f_conv_plan;
/* the plans d3f_conv_forward, d3f_conv_backward_data (upsample0 == 2: with the 2x2-summed request) and
 * d3f_conv_backward_weight make of (dtype, d); with_workspace: as if the two former were handed their split-K workspace.
 * < 0: a description no entry accepts (dtype, extents, channel multiples). */
int d3f_conv_layer_plan(int dtype, const d3f_conv_desc* d, int with_workspace, d3f_conv_plan* out);
/* the convolution layers of a network handle, in launch order (d3f_unet_plan_counts counts the same units), as the engine
 * planned them: its own plan_nets, split-K workspace and 2x2-summed request (d->upsample0 == 2 where the source is
 * up-sampled).  The segmentation head (the last layer) runs its forward with the bias + NCHW epilogue. */
int d3f_unet_num_conv_layers(d3f_unet_t h);
int d3f_unet_conv_layer(d3f_unet_t h, int i, d3f_conv_desc* d, d3f_conv_plan* plan);

/* BatchNorm2d, train mode (eps 1e-5, momentum 0.1): finalize conv statistics, then
 * a = relu?(y*scale + shift + residual); coef = mean[C] invstd[C] scale[C] shift[C] */
int d3f_bn_finalize(const float* stats, int tiles, int C, int64_t count, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, float* coef, void* stream);
int d3f_bn_apply(int dtype, const void* y, const float* coef, int C, int64_t rows, const void* residual,
                 int relu, void* out, void* stream);
/* backward of a = relu?(bn(y) + residual): dy, dgamma, dbeta, and (dres != NULL) dz for the residual */
size_t d3f_bn_backward_workspace_bytes(int dtype, int C, int64_t rows);
int d3f_bn_backward(int dtype, const void* dA, const void* a_or_null, const void* y, const float* coef,
                    const float* gamma, int C, int64_t rows, void* dy, void* dres, float* dgamma,
                    float* dbeta, void* workspace, void* stream);

/* One BatchNorm layer as the engine describes, plans and launches it: the description below is planned into the fused
 * form (the finalize step folded into the streaming pass: fp32 / bf16, C a multiple of 32, 1..1024 partial rows,
 * allow_fused) or the split form, and a pass is ONE call that runs the planned form -- the same two calls the network
 * makes.  The three entry points above keep building the split form only. */
typedef struct d3f_bn_desc {
  int32_t dtype, C, Cpad; /* storage dtype; channels; stride (channels) of the forward statistics rows, >= C */
  int64_t rows;           /* rows (pixels) of y */
  int32_t apply, relu;    /* apply 0: coefficients and running statistics only (a downsample branch; `a` is not written) */
  int32_t res;            /* 0 none, 1 + a tensor, 2 + another layer's y * scale + shift (its coefficient block) */
  int32_t mask;           /* backward ReLU mask: 0 none, 1 recomputed as y * scale + shift > 0, 2 read as a > 0 */
  int32_t fwd_rows;       /* forward partial rows the caller hands in: (sum, sum of squares) per channel, [fwd_rows][Cpad][2] */
  int32_t fused_rows;     /* > 0: backward partial rows the caller hands in: (sum dz, sum dz * xhat), [fused_rows][C][2];
                           * 0: the backward pass reduces dz itself into `partial` */
  int32_t allow_fused, plan_nets; /* plan_nets 1 or 2: networks whose workgroups the fused passes count */
} d3f_bn_desc;
typedef struct d3f_bn_plan {
  int32_t fwd_fused, bwd_fused; /* finalize folded into the streaming pass */
  int32_t reduce_blocks;        /* partial rows the backward's own reduce writes (1..1024) */
  int32_t bwd_rows;             /* partial rows the backward reads: fused_rows, or reduce_blocks */
  int64_t rows_per_block;       /* rows per workgroup of the fused passes (0: neither pass is fused) */
  uint64_t stat_floats;         /* floats the forward reads from `stats` */
  uint64_t part_floats;         /* floats `partial` must hold */
} d3f_bn_plan;
#define D3F_BN_COEF_ROWS 7 /* a coefficient block: mean invstd scale shift k0 k1 k2, C floats each */
/* host only (no GPU): validates the description and plans it */
int d3f_bn_layer_plan(const d3f_bn_desc* d, d3f_bn_plan* plan);
/* stats -> rows 0..3 of coef, running statistics (both NULL: not tracked), and with apply
 * a = relu?(y * scale + shift [+ res | + res * scale_r + shift_r]).  res_coef: the other layer's block (res == 2).
 * rows == 0: nothing is launched.  A description the planned form's kernels cannot run is D3F_EINVAL (-1). */
int d3f_bn_layer_forward(const d3f_bn_desc* d, float* stats, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float* coef, const void* y, const void* res, const float* res_coef, void* a,
                         void* stream);
/* dz = dA * mask; partial (part_floats floats: read with fused_rows > 0, else scratch) -> dgamma, dbeta (both NULL: not
 * wanted), rows 4..6 of coef, dy, and dres (NULL: not wanted) = dz, or += dz with dres_acc.  coef: the block the forward
 * pass filled; a: the activation (mask == 2). */
int d3f_bn_layer_backward(const d3f_bn_desc* d, float* partial, const float* gamma, float* coef, const void* y,
                          const void* a, const void* dA, void* dy, void* dres, int dres_acc, float* dgamma, float* dbeta,
                          void* stream);
/* the description and plan the engine holds for BatchNorm layer i (d3f_unet_bn_info's order); host only */
int d3f_unet_bn_layer(d3f_unet_t h, int i, d3f_bn_desc* d, d3f_bn_plan* plan);

/* The head activation's two launches as the engine makes them (D3F_ACT_* above; smp's Activation behind
 * SegmentationHead, d3f/train_denoiser/lit_module.py:46-52).  forward: a = act(z), both NCHW f32 [B][C][H][W].
 * backward: (z, g = d loss / d a) -> dz, written twice by one launch: dz_nchw NCHW f32 (the bias gradient's channel sum
 * reads it) and dy_nhwc [B][H][W][Cpad] in the storage dtype, rounded once from the f32 dz, channels [C, Cpad) zero
 * (the head's data and weight gradients read it); dz_nchw may be z itself.  C < 1, C > 16, Cpad < C and an unknown act are D3F_EINVAL (-1)
 * before anything is enqueued. */
int d3f_head_activation_forward(int act, const float* z, float* a, int B, int C, int H, int W, void* stream);
int d3f_head_activation_backward(int act, int dtype, const float* z, const float* g, float* dz_nchw, void* dy_nhwc,
                                 int B, int C, int H, int W, int Cpad, void* stream);

int d3f_maxpool3x3s2_forward(int dtype, const void* in, void* out, uint8_t* idx, int B, int H, int W, int C, void* stream);
int d3f_maxpool3x3s2_backward(int dtype, const void* dout, const uint8_t* idx, void* din, int accumulate,
                              int B, int H, int W, int C, void* stream);
int d3f_upsample2x_backward(int dtype, const void* dfull, void* dlow, int B, int Hlow, int Wlow, int C, void* stream);
int d3f_nchw_to_nhwc(int dtype, const float* in, void* out, int B, int C, int H, int W, int Cpad, void* stream);
int d3f_nhwc_to_nchw(int dtype, const void* in, float* out, int B, int C, int H, int W, int Cpad, void* stream);
/* Host half of the input pipeline moved to the device (d3f/train_deep_fake/lit_module.py:100-110: A.Normalize(mean, std,
 * max_pixel_value=255) + ToTensorV2 on the HWC uint8 RGB image d3f/dataset/image_dataset.py:37-41 hands the transform):
 * in_hwc [B][H][W][3] uint8 RGB -> out_nchw [B][3][H][W] f32 = ((float)u8 / 255 - mean[c]) / std[c], the transform's
 * own order of fp32 operations (bit-identical); the batch crosses worker IPC and PCIe as bytes. */
int d3f_u8rgb_normalise(const uint8_t* in_hwc, float* out_nchw, int B, int H, int W, const float mean[3],
                        const float std[3], void* stream);

/* crop_image_at_center + resize_image of the script tools (d3f/script_tools/put_video_through_fake_model.py:121-145,
 * video_to_center_cropped_images.py:83-107): the crop box (x1, y1, cw, ch) of src [B][src_h][src_w][3] uint8 (any
 * channel order) resized to dst [B][H][W][3] uint8 whose rows lie dst_row_stride_bytes apart (>= 3 * W; frames H rows
 * apart) -- 6 * W writes the left half of a side-by-side frame.  The resize is cv2.INTER_CUBIC in float arithmetic:
 * source coordinate f = (d + 0.5) * n_in / n_out - 0.5 computed exactly (integers), taps floor(f) - 1 .. floor(f) + 2
 * clamped to the crop (replicate border), Keys weights with A = -0.75, no antialiasing, horizontal then vertical pass in
 * fp32, rintf (half to even), clamp to 0..255; equal extents copy the bytes.  OpenCV's own 8-bit path uses 11-bit
 * fixed-point coefficients and may differ from this definition by one level on some pixels: byte equality with OpenCV
 * is not claimed.  Refused: a box outside the frame, non-positive sizes, extents above 16384, a stride below 3 * W. */
int d3f_crop_resize_cubic_u8(const uint8_t* src, int B, int src_h, int src_w, int x1, int y1, int cw, int ch, uint8_t* dst,
                             int H, int W, int64_t dst_row_stride_bytes, void* stream);
/* d3f_crop_resize_cubic_u8 with antialiasing: arguments, layouts and refusals are its own, the filter is Pillow's bicubic,
 * which is also torch.nn.functional.interpolate(mode="bicubic", antialias=True, align_corners=False): an axis that shrinks
 * by r = n_in / n_out widens the Keys kernel by r, so that every source pixel of an output pixel's footprint is read.
 * Definition (the acceptance contract; tests/resize_aa_restatement.py restates it in float64).  Per axis n_in -> n_out,
 * output index i, everything up to the weights' arguments in exact integers:
 *   - down = n_in >= n_out; centre c = (2i + 1) n_in / (2 n_out); support s = 2 n_in / n_out when down, else 2;
 *   - with S = 4 n_in when down, else 4 n_out: first tap xmin = max(floor(((2i + 1) n_in - S + n_out) / (2 n_out)), 0), end
 *     xmax = min(floor(((2i + 1) n_in + S + n_out) / (2 n_out)), n_in); taps k = xmin .. xmax - 1, at most
 *     floor(S / n_out) + 1 of them.  The window is TRUNCATED at the crop's edge, not replicated;
 *   - raw weight w_k = keys(|a_k|), a_k = ((2k + 1) n_out - (2i + 1) n_in) / D, D = 2 n_in when down, else 2 n_out: the
 *     numerator is an exact integer below 2^24 in magnitude for extents up to 16384, so ONE fp32 division rounds a_k
 *     correctly; keys with A = -0.5 in fp32, Horner form: ((A + 2) x - (A + 3)) x x + 1 for x < 1,
 *     ((A x - 5A) x + 8A) x - 4A for 1 <= x < 2, 0 from 2 on;
 *   - the weights' sum, in fp32: with t = k - xmin, eight sums p_j over the taps t = j, j + 8, j + 16, ... in that order
 *     (0 when there is none), sum = ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)); the weight of tap k is the fp32
 *     quotient w_k / sum.
 * The two passes, in fp32 without contraction (no fma), over the crop:
 *   - horizontal: for a source row, four sums q_u over the taps t = u, u + 4, u + 8, ... of weight * (float)byte, each
 *     started from 0 and taken in that order, h = (q0 + q1) + (q2 + q3);
 *   - vertical: the source rows are taken in chunks of 8 counted from ymin of the first output row of the pixel's tile of 8
 *     output rows (row 8 floor(i_y / 8)); inside a chunk the products weight * h of the rows in the pixel's window are
 *     added in row order from 0, and the chunk's sum is added to the running value, chunks in order;
 *   - rintf (half to even), clamp to 0..255.
 * Equal extents on an axis give weight 1 on tap i and exact zeros elsewhere (a = -1, 0, 1, 2); equal extents on both axes
 * therefore copy the bytes, as the plain operator does.  An axis that ENLARGES gets Pillow's up-sampling -- A = -0.5, the
 * window truncated at the edge and renormalised -- and not cv2's (A = -0.75, replicated border) as in
 * d3f_crop_resize_cubic_u8: deliberately, the mode is one filter whatever the direction, and it is the one torch computes.
 * Refused on the host before any launch: everything d3f_crop_resize_cubic_u8 refuses, and a crop extent above 32 times the
 * output extent on either axis (n_in > 32 n_out: the limit caps an axis at 129 taps; 2160 -> 128 is 16.9 and fits). */
int d3f_crop_resize_cubic_aa_u8(const uint8_t* src, int B, int src_h, int src_w, int x1, int y1, int cw, int ch,
                                uint8_t* dst, int H, int W, int64_t dst_row_stride_bytes, void* stream);
/* The inverse of d3f_crop_resize_cubic_u8 with a blend in the epilogue: paste a patch back into the frames it was cropped
 * from.  patch [B][H][W][3] uint8, rows patch_row_stride_bytes apart (>= 3 * W; frames H rows apart; 6 * W reads the right
 * half of a pair_out buffer); frame and out [B][src_h][src_w][3] uint8, packed; (x1, y1, cw, ch) the box the crop was taken
 * from.  Definition (the acceptance contract; tests/paste_restatement.py restates it in float64):
 *   - outside the box: out is the byte of frame;
 *   - inside, at box pixel (i, j), row i in [0, ch), column j in [0, cw): v = the fp32 value of d3f_crop_resize_cubic_u8's
 *     definition for the resize H x W -> ch x cw of the whole patch (the same exact integer source coordinates, Keys
 *     weights with A = -0.75, taps clamped inside the patch, horizontal then vertical pass in fp32 without contraction --
 *     the same device functions), taken BEFORE that operator's rintf; then v = fminf(fmaxf(v, 0), 255);
 *   - the ramp, per axis: d_y = min(i, ch - 1 - i), a_y = (float)min(d_y + 1, feather + 1) / (float)(feather + 1) (one
 *     IEEE fp32 division of exact integers), a_x likewise from j and cw, a = a_y * a_x;
 *   - the blend: o = a * v + (1.f - a) * s with s the frame's byte, both products and the sum rounded separately; the byte
 *     is rintf(o) (half to even) clamped to 0..255.  Where a == 1 that is rintf(v): the byte
 *     d3f_crop_resize_cubic_u8(patch -> ch x cw) writes.  feather == 0: the whole box is that.
 * out == frame runs in place (a lane reads only the frame bytes it writes; only the tiles that meet the box are
 * launched); with out != frame one launch covers the whole frame.  Refused before any device call: null pointers, B < 0
 * or B > 65535 (B == 0 launches nothing), non-positive sizes, a box outside the frame, extents above 16384, feather < 0
 * or > 16384, a patch stride below 3 * W, frame and out that overlap in part, a patch whose bytes (first pixel of the first patch to
 * last pixel of the last) overlap out -- a tile reads its part of the patch while other tiles write out. */
int d3f_paste_resize_cubic_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                              const uint8_t* frame, int src_h, int src_w, int x1, int y1, int cw, int ch, int feather,
                              uint8_t* out, void* stream);

/* Colour match of a pasted patch: mean / std (Reinhard) matching per frame and per byte-in-pixel, in three operators.  The
 * definitions are the acceptance contract; tests/color_match_restatement.py restates them (sums with Python integers,
 * coefficients in float64, the paste on top of tests/paste_restatement.py).
 *
 * d3f_channel_sums_u8: img [B][H][W][3] uint8, rows row_stride_bytes apart (>= 3 * W; frames H rows apart; 6 * W reads one
 * half of a pair_out buffer), from any byte address.  sums [B][3][2] uint64: for frame b and byte-in-pixel c, S = sum of p and
 * Q = sum of p * p over all n = H * W pixels, exact.  The call OVERWRITES sums: the reset of the accumulators is part of the
 * enqueued work, so a captured call replayed on new bytes gives the new sums.  Refused before any device call: null
 * pointers, B < 0 or B > 65535 (B == 0 launches nothing), non-positive sizes, a stride below 3 * W, H * W > 2^22 (the limit
 * keeps n * Q and S * S below 2^60, so the next step is exact in 64-bit integers). */
int d3f_channel_sums_u8(const uint8_t* img, int B, int H, int W, int64_t row_stride_bytes, uint64_t* sums, void* stream);
/* d3f_color_match_coef: sums_from, sums_to [B][3][2] uint64 as above, both over n pixels -> coef [B][3][2] fp32, gain then
 * offset, such that gain * p + offset takes the mean and standard deviation of `from` to those of `to`.  Per (b, c), in
 * float64:
 *   - D = n * Q - S * S as exact uint64, for from and to; m = (double)S / (double)n for each;
 *   - g = 1 if D_from == 0 or D_to == 0, else sqrt((double)D_to / (double)D_from);
 *   - g = fmin(fmax(g, D3F_COLOR_GAIN_MIN), D3F_COLOR_GAIN_MAX): a design choice, not a measurement -- it keeps a nearly flat
 *     frame from amplifying noise eight-fold;
 *   - o = m_to - g * m_from, product and difference rounded separately; coef = (float)g, (float)o.
 * Refused before any device call: null pointers, B < 0 or B > 65535 (B == 0 launches nothing), n <= 0 or n > 2^22. */
#define D3F_COLOR_GAIN_MIN 0.5
#define D3F_COLOR_GAIN_MAX 2.0
int d3f_color_match_coef(const uint64_t* sums_from, const uint64_t* sums_to, int B, int64_t n, float* coef, void* stream);
/* d3f_paste_resize_cubic_color_u8: d3f_paste_resize_cubic_u8 with one insertion.  coef [B][3][2] fp32 in device memory; at
 * frame b, byte-in-pixel c, after v = fminf(fmaxf(v, 0), 255): w = coef[b][c][0] * v (rounded), w = w + coef[b][c][1]
 * (rounded), w = fminf(fmaxf(w, 0), 255), and the blend takes w where it took v.  Ramp, blend, in-place form, tile selection
 * and refusals are those of d3f_paste_resize_cubic_u8 (the same kernel with one more template parameter); a null coef and a
 * coef whose B * 24 bytes overlap out are refused too.  Coefficients (1, 0) give d3f_paste_resize_cubic_u8's bytes. */
int d3f_paste_resize_cubic_color_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                    const uint8_t* frame, int src_h, int src_w, int x1, int y1, int cw, int ch, int feather,
                                    const float* coef, uint8_t* out, void* stream);

/* A box per frame: a face that moves through the frames.  Each of the four operators below is the signature of its single-box
 * operator with x1, y1, cw, ch replaced by boxes: HOST memory, [B][4] int32 as x1, y1, cw, ch of frame b, read before the call
 * returns (the caller may free or change it then).  Definition by reference: frame b of the result is byte for byte what the
 * single-box operator gives on frame b alone (B = 1) with box b -- the same device functions run on the same operands; the
 * per-frame form is still one device call.  The boxes travel by value in the kernels' arguments, D3F_FRAME_BOXES_MAX of them
 * (1 KB) per launch: there is no device copy of them and no device-side read of a box that was not checked; a call with more
 * frames is several launches of at most D3F_FRAME_BOXES_MAX frames, enqueued in order.  The paste keeps ONE feather for the
 * call.  Refused before any device call: a null boxes with B > 0; for ANY frame, whatever the single-box operator refuses of
 * one box -- a non-positive extent, a box outside the frame, for the antialiased form an extent above 32 times the output's
 * -- with the frame's index in the message; and whatever else the single-box operator refuses (pointers, sizes, strides,
 * overlaps, feather). */
#define D3F_FRAME_BOXES_MAX 64
/* d3f_crop_resize_cubic_u8 with boxes */
int d3f_crop_resize_cubic_boxes_u8(const uint8_t* src, int B, int src_h, int src_w, const int32_t* boxes, uint8_t* dst, int H,
                                   int W, int64_t dst_row_stride_bytes, void* stream);
/* d3f_crop_resize_cubic_aa_u8 with boxes */
int d3f_crop_resize_cubic_aa_boxes_u8(const uint8_t* src, int B, int src_h, int src_w, const int32_t* boxes, uint8_t* dst,
                                      int H, int W, int64_t dst_row_stride_bytes, void* stream);
/* d3f_paste_resize_cubic_u8 with boxes.  out == frame runs in place: of every frame only the tiles that meet ITS box are
 * written (one grid for the launch, the largest tile count of any of its frames; a frame's workgroups past its own count
 * return at once), so bytes outside a frame's own box stay untouched. */
int d3f_paste_resize_cubic_boxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                    const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, int feather,
                                    uint8_t* out, void* stream);
/* d3f_paste_resize_cubic_color_u8 with boxes (coef [B][3][2] stays device memory) */
int d3f_paste_resize_cubic_color_boxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                          const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, int feather,
                                          const float* coef, uint8_t* out, void* stream);

/* Rotated boxes: a face whose head rolls.  Each operator below is its _boxes_ operator with one more table, rot: HOST memory,
 * [B][2] int32 as c16 = round(cos a * 65536), s16 = round(sin a * 65536) of frame b's angle a, read before the call returns.
 * Coordinates are x right, y down; a positive angle turns the box clockwise on the screen about its centre: in frame
 * coordinates the crop's column direction is (cos a, sin a), its row direction (-sin a, cos a).  No trigonometry on the
 * device: the two integers are the rotation (ops.box_rotation computes them from an angle in degrees).  Definition (the
 * acceptance contract; tests/rotation_restatement.py restates it), with c = c16 / 65536, s = s16 / 65536 and the box's centre
 * (X, Y) = (x1 + (cw - 1) / 2, y1 + (ch - 1) / 2) in tap-index units:
 *   crop: output pixel (ox, oy) of the H x W crop reads the FRAME at (X + c u - s v, Y + s u + c v) with
 *     u = cw (2 ox + 1 - W) / (2 W), v = ch (2 oy + 1 - H) / (2 H).  Each coordinate is formed exactly in 64-bit integers over
 *     the denominator 2^17 W H and reduced once, by a floor, to a fixed-point position with 16 fractional bits: its integer
 *     part is s, its fraction t = frac / 65536 exact in fp32.  Taps s - 1 .. s + 2 per axis, Keys weights (A = -0.75) of t as
 *     in d3f_crop_resize_cubic_u8, horizontal then vertical pass in fp32 without contraction, rintf, clamp.  Tap indices are
 *     clamped to the FRAME (replicate), not to the box: a rotated box's corners may leave the frame, and no read ever does.
 *     This is a stated difference from the plain form, and angle 0 is therefore (and for the 16-bit fraction) not promised
 *     byte-equal to d3f_crop_resize_cubic_boxes_u8: it differs by at most one level away from the box's border ring.
 *   paste: for frame pixel p = (x, y), dx2 = 2 x - 2 x1 - cw + 1, dy2 = 2 y - 2 y1 - ch + 1, the box-local position is
 *     j' = n_j / 2^17, i' = n_i / 2^17 with n_j = (cw - 1) 2^16 + c16 dx2 + s16 dy2, n_i = (ch - 1) 2^16 - s16 dx2 + c16 dy2
 *     (exact integers).  The pixel belongs to the box when -0.5 <= j' < cw - 0.5 and -0.5 <= i' < ch - 0.5 (tested on n_j,
 *     n_i); every other byte of out is the frame's.  The patch is sampled at (j' + 0.5) W / cw - 0.5 -- exactly
 *     ((n_j + 2^16) W - 2^16 cw) / (2^17 cw), reduced by a floor to 16 fractional bits -- and likewise for i'; taps clamped
 *     inside the patch; value, clamp, colour form and blend exactly as d3f_paste_resize_cubic_u8 / _color_u8.  The ramp of an
 *     axis: f = floor(n_j / 2), d = min(f, (cw - 1) 2^16 - f), a_x = (float)min(d + 2^16, (feather + 1) 2^16) /
 *     (float)((feather + 1) 2^16) (two integers converted to fp32, one division), a = a_y * a_x.  At angle 0 it is the plain
 *     form's ramp.
 * The tables travel by value (box and rotation: 1.5 KB per launch of at most D3F_FRAME_BOXES_MAX frames; a longer call is
 * several launches, in order).  A tile stages the axis-aligned bounding box of its footprint, clipped to the image; a launch
 * whose largest footprint passes 32 KB reads its taps from global memory with the same arithmetic, and both routes give the
 * same bytes.  The in-place paste launches only the tiles that meet the rotated rectangle's bounding box.
 * Refused before any device call: whatever the _boxes_ operator refuses (the box itself lies inside the frame), a null rot,
 * and for any frame a rot with |c16^2 + s16^2 - 2^32| > 2^17 -- such a table would scale, not rotate -- with the frame's index
 * in the message.  Extents up to 16384 as ever: no intermediate passes 2^60. */
int d3f_crop_resize_cubic_rboxes_u8(const uint8_t* src, int B, int src_h, int src_w, const int32_t* boxes, const int32_t* rot,
                                    uint8_t* dst, int H, int W, int64_t dst_row_stride_bytes, void* stream);
/* the fused form the frame entries launch: dst as above and, from the same rounded bytes, the normalised activation
 * act [B][H][W][Cpad] (dtype D3F_F32 or D3F_BF16, device memory, Cpad >= 3) in RGB order: ((float)byte - mean[c] * 255.f) /
 * (std[c] * 255.f) in fp32, channels from 3 on zero; mean, std: 3 host floats (RGB order) */
int d3f_crop_resize_cubic_rboxes_u8_nhwc(int dtype, const uint8_t* src, int B, int src_h, int src_w, const int32_t* boxes,
                                         const int32_t* rot, uint8_t* dst, int H, int W, int64_t dst_row_stride_bytes,
                                         void* act, int Cpad, const float mean[3], const float std[3], void* stream);
int d3f_paste_resize_cubic_rboxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                     const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, const int32_t* rot,
                                     int feather, uint8_t* out, void* stream);
int d3f_paste_resize_cubic_color_rboxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                           const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, const int32_t* rot,
                                           int feather, const float* coef, uint8_t* out, void* stream);

/* Multiband paste (Burt & Adelson): d3f_paste_resize_cubic_u8 with the single ramp replaced by a ramp per spatial frequency
 * band -- low frequencies fade over about `feather` pixels, every finer band over half the band above.  Inputs: those of
 * d3f_paste_resize_cubic_u8 (with coef: of d3f_paste_resize_cubic_color_u8), levels = N in 1..D3F_MULTIBAND_MAX_LEVELS, and a
 * workspace in device memory.  Definition (the acceptance contract; tests/multiband_restatement.py restates it in numpy
 * integers; every comparison is exact), per frame and byte-in-pixel, all in integers:
 *   - V[i][j], the target byte: what d3f_paste_resize_cubic_u8 (with coef: d3f_paste_resize_cubic_color_u8) writes at box
 *     pixel (i, j) with feather = 0 -- rintf of the clamped fp32 resize value, from the same device functions;
 *   - D = V - s in -255..255, s the frame's byte; g_0 = D << 6, held in int16.  Outside the box D is zero by definition;
 *   - level sizes: h_0 = ch, w_0 = cw, h_{l+1} = (h_l + 1) / 2, w likewise;
 *   - REDUCE: g_{l+1}[i][j] = (sum over a, b in -2..2 of w_a w_b g_l[clamp(2i + a)][clamp(2j + b)] + 128) >> 8 with
 *     w = 1 4 6 4 1, indices clamped into level l, the sum exact, the shift arithmetic (floor);
 *   - EXPAND of a level to h_l x w_l: per axis, output index 2k takes g[k - 1] + 6 g[k] + g[k + 1], output index 2k + 1 takes
 *     4 g[k] + 4 g[k + 1], indices clamped into the coarse level; the 2-D value is the product form of the two axes (the
 *     weights sum to 64): (sum + 32) >> 6, arithmetic shift;
 *   - band masks: F = (feather + (1 << N) - 1) >> N, the ramp's width in SAMPLES of every level.  At level l,
 *     n_y(i) = min(min(i, h_l - 1 - i) + 1, F + 1), n_x likewise, M = n_y n_x, den = (F + 1)^2 and
 *     m_l(x) = floor((2 x M + den) / (2 den)) (floor also for negative x; where M == den this is x);
 *   - collapse: R_N = m_N(g_N); for l = N - 1 .. 0: R_l = EXPAND(R_{l+1}) + m_l(g_l - EXPAND(g_{l+1})), R in int32;
 *   - E = (R_0 + 32) >> 6; the byte in the box is clamp(s + E, 0, 255), outside the box the frame's byte.
 * Consequences: feather == 0 gives F == 0, every mask is the identity, each level adds back the very expansion it
 * subtracted, E == D and out is byte for byte d3f_paste_resize_cubic_u8 with feather = 0; a patch whose resize equals the
 * frame in the box (D == 0) returns the frame.
 * workspace: d3f_paste_multiband_workspace_bytes(B, cw_max, ch_max, levels) bytes (cw_max, ch_max: the largest box extents of
 * the call; < 0 for arguments it refuses) starting on 16 bytes; its contents before the call do not matter and are undefined
 * after it.  2 N + 1 launches (per 64 frames in the boxes forms).  out == frame runs in place under
 * d3f_paste_resize_cubic_u8's rules: the last launch reads no frame byte but the three it writes.  The boxes forms: frame b is
 * byte for byte the single-box call on frame b with box b.  Refused before any device call: everything the plain (colour,
 * boxes) paste refuses, levels outside 1..6, a box with min(cw, ch) < (1 << N) (the boxes forms name the frame), a null,
 * misaligned or short workspace, a workspace that overlaps patch, frame, out or coef. */
#define D3F_MULTIBAND_MAX_LEVELS 6
int64_t d3f_paste_multiband_workspace_bytes(int B, int cw_max, int ch_max, int levels);
int d3f_paste_multiband_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes, const uint8_t* frame,
                           int src_h, int src_w, int x1, int y1, int cw, int ch, int feather, int levels, void* workspace,
                           int64_t workspace_bytes, uint8_t* out, void* stream);
int d3f_paste_multiband_color_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                 const uint8_t* frame, int src_h, int src_w, int x1, int y1, int cw, int ch, int feather,
                                 int levels, const float* coef, void* workspace, int64_t workspace_bytes, uint8_t* out,
                                 void* stream);
int d3f_paste_multiband_boxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                 const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, int feather, int levels,
                                 void* workspace, int64_t workspace_bytes, uint8_t* out, void* stream);
int d3f_paste_multiband_color_boxes_u8(const uint8_t* patch, int B, int H, int W, int64_t patch_row_stride_bytes,
                                       const uint8_t* frame, int src_h, int src_w, const int32_t* boxes, int feather,
                                       int levels, const float* coef, void* workspace, int64_t workspace_bytes, uint8_t* out,
                                       void* stream);

/* Temporal filter against flicker in the fake video, in two operators.  The definitions are the acceptance contract;
 * tests/temporal_restatement.py restates them in numpy float32 and int64, and every comparison is exact.  All fp32 arithmetic
 * is single operations without contraction, integer-to-float conversions are exact, the division is the correctly rounded one.
 * The defaults (D3F_TEMPORAL_STRENGTH, D3F_TEMPORAL_THRESHOLD, D3F_TEMPORAL_CUT_LEVELS) are design choices, not measurements.
 *
 * d3f_temporal_filter_u8: a motion-gated recursive filter on the fake.  real [B][H][W][3] uint8, rows real_row_stride_bytes
 * apart, frames H rows apart, any byte address; fake the same with its own stride, filtered IN PLACE (6 * W and a fake 3 * W
 * bytes behind real: the halves of a pair_out buffer).  State, in device memory: state_fake [H][W][3] fp32, state_real
 * [H][W][3] uint8 packed, state_valid int32[1].  The frames of a call are consecutive in time: frame b's predecessor is frame
 * b - 1, frame 0's is the state.  For frame b at pixel (i, j), with r the real frame, r_prev the predecessor's, f the fake's
 * bytes and S_prev the predecessor's filtered value (fp32):
 *   - sad = sum over dy, dx in {-1, 0, 1} and the 3 bytes of a pixel of |r[cy][cx][c] - r_prev[cy][cx][c]|, cy = clamp(i + dy,
 *     0, H - 1), cx = clamp(j + dx, 0, W - 1): replicated border, always 27 terms, an exact integer in 0..6885;
 *   - T = 27 * threshold, k = strength * ((float)max(T - sad, 0) / (float)T): one k per pixel for its three bytes;
 *   - per byte d = S_prev - (float)f, p = k * d, S = (float)f + p; the byte written is rintf(S) clamped to 0..255, and S,
 *     unrounded, is the successor's S_prev.  k == 0 (the surroundings moved) keeps the fake's byte bit for bit;
 *   - with no valid predecessor (*state_valid == 0 and b == 0) S = (float)f, and neither state buffer is read: they may
 *     hold anything, NaN included.
 * The gate reads the REAL crop: the fake changing where its input did not is the flicker, the fake changing where the input
 * moved is the signal.  A cut needs no detector: after one nearly every pixel has sad >= T and passes through.
 * After a call state_fake holds the last frame's S, state_real its real bytes, and state_valid is 1 -- set by a small launch
 * enqueued BEHIND the kernel on the stream, so a captured call replays correctly.  To reset, store 0 to state_valid on the
 * same stream.  B == 0 touches nothing.  Refused before any device call: null pointers, B < 0 or B > 65535, sizes outside
 * 1..16384, strength outside [0, 1) or NaN, threshold outside 1..255, a row stride below 3 * W, a state_fake or state_valid
 * that is not 4-byte aligned, and any overlap between real, fake and the state buffers (real and fake may interleave row by
 * row with one stride, as the halves of a pair buffer do). */
#define D3F_TEMPORAL_STRENGTH 0.75f
#define D3F_TEMPORAL_THRESHOLD 8
#define D3F_TEMPORAL_CUT_LEVELS 16
int d3f_temporal_filter_u8(const uint8_t* real, int64_t real_row_stride_bytes, uint8_t* fake, int64_t fake_row_stride_bytes,
                           int B, int H, int W, float* state_fake, uint8_t* state_real, int32_t* state_valid, float strength,
                           int threshold, void* stream);
/* d3f_color_coef_smooth: d3f_color_match_coef's coefficients smoothed across frames, in place.  coef [B][3][2] fp32 (gain,
 * offset); sums_to [B][3][2] uint64, the real crop's d3f_channel_sums_u8, of which only S = [..][0] is read; n pixels per frame.
 * State: state_coef [3][2] fp32, state_sum [3] uint64, state_valid int32[1].  For the frames in order:
 *   - cut = the predecessor is invalid, or for any channel |S[c] - S_prev[c]| > D3F_TEMPORAL_CUT_LEVELS * n in exact 64-bit
 *     integers (the crop's mean moved by more than 16 levels);
 *   - at a cut c = c' exactly and the state is not read; otherwise c = c' + strength * (c_prev - c'): difference, product
 *     and sum rounded separately;
 *   - coef[b] = c, and the state becomes (c, S).
 * state_valid is set behind the launch, as above; B == 0 touches nothing.  Refused: null pointers, B < 0 or B > 65535,
 * n <= 0 or n > 2^22, strength outside [0, 1) or NaN. */
int d3f_color_coef_smooth(float* coef, const uint64_t* sums_to, int B, int64_t n, float strength, float* state_coef,
                          uint64_t* state_sum, int32_t* state_valid, void* stream);
/* *flag = value by a one-lane launch on the stream: the reset of either operator's state (value 0). */
int d3f_temporal_flag_set(int32_t* flag, int value, void* stream);

/* Template tracker: the face box of a --track file from boxes set by hand at key frames, with no detector.  Integer
 * arithmetic throughout, so the result does not depend on the order of evaluation; tests/track_restatement.py restates it in
 * numpy and Python integers and every comparison is exact.  The defaults (D3F_TRACK_TEMPLATE_SIDE, _SEARCH, _ADAPT, _LOST) are
 * design choices, not measurements.  The plain entries follow a template of fixed size; the _scale_ entries below search
 * the size too, the _rot_ entries below them head roll.
 *
 * d3f_gray_decimate_u8: frames [B][h][w][3] uint8 BGR, packed, any byte address -> out [B][gh][gw] uint8, gh = h / s,
 * gw = w / s (partial blocks at the right and bottom are dropped), out[y][x] = (sum over the s x s block of B + 2 G + R) /
 * (4 s s) in integers.  gh == 0 or gw == 0 writes nothing.  No dword is loaded whole outside the frames' bytes, and no byte
 * outside out is written.
 * d3f_track_seed_u8: that grey of the box (tx, ty, tw, th) of ONE frame's reduced image -> templ, tw bytes a row, th rows,
 * packed at the front of a buffer of D3F_TRACK_MAX_SIDE * D3F_TRACK_MAX_SIDE bytes; pos int32[2] = (tx, ty).
 * d3f_track_search_u8: gray [B][gh][gw], the frames of a call consecutive in time; templ and pos are read at the start and
 * written at the end (a pos outside 0..gw - tw, 0..gh - th is moved inside first).  For each frame in order:
 *   - candidates (dx, dy) in [-search, search]^2 with 0 <= pos.x + dx <= gw - tw and 0 <= pos.y + dy <= gh - th;
 *   - cost = sum over the template of |gray[pos.y + dy + j][pos.x + dx + i] - templ[j][i]|, below 2^20;
 *   - key = cost << 32 | (dx dx + dy dy) << 16 | (dy + search) << 8 | (dx + search), unsigned 64 bits; the smallest key wins
 *     (equal costs: the smaller displacement, then the smaller dy, then the smaller dx);
 *   - found = cost <= lost * tw * th.  Found: pos += (dx, dy), then templ = (templ * (8 - adapt) + window * adapt + 4) >> 3 per
 *     sample with the window at the new pos.  Not found: pos and templ stay exactly as they were;
 *   - out[b] = (pos.x, pos.y, cost, found), pos after the update.
 * A reduced position (px, py) is the face (px * s + ox, py * s + oy, fw, fh) of the seed's geometry (the Python side:
 * ops.track_template_geometry).
 * d3f_track_template_u8: d3f_gray_decimate_u8 of the frames into gray_ws [B][gh][gw], then d3f_track_search_u8 on it: two
 * launches in one call.
 * B == 0 touches nothing.  Refused before any device call: null pointers, B < 0 or B > 65535, sizes outside 1..16384, s outside
 * 1..D3F_TRACK_MAX_STRIDE, tw or th outside 4..D3F_TRACK_MAX_SIDE, a template larger than the reduced image (gh < th, gw < tw)
 * or a seed box outside it, search outside 1..D3F_TRACK_MAX_SEARCH, adapt outside 0..8, lost outside 0..255, a pos or out
 * that is not 4-byte aligned. */
#define D3F_TRACK_MAX_SIDE 64
#define D3F_TRACK_MAX_SEARCH 64
#define D3F_TRACK_MAX_STRIDE 32
#define D3F_TRACK_TEMPLATE_SIDE 48
#define D3F_TRACK_SEARCH 16
#define D3F_TRACK_ADAPT 1
#define D3F_TRACK_LOST 16
int d3f_gray_decimate_u8(const uint8_t* frames, int B, int h, int w, int s, uint8_t* out, void* stream);
int d3f_track_seed_u8(const uint8_t* frame, int h, int w, int s, int tx, int ty, int tw, int th, uint8_t* templ, int32_t* pos,
                      void* stream);
int d3f_track_search_u8(const uint8_t* gray, int B, int gh, int gw, int tw, int th, int search, int adapt, int lost,
                        uint8_t* templ, int32_t* pos, int32_t* out, void* stream);
int d3f_track_template_u8(const uint8_t* frames, int B, int h, int w, int s, int tw, int th, int search, int adapt, int lost,
                          uint8_t* templ, int32_t* pos, uint8_t* gray_ws, int32_t* out, void* stream);

/* Template tracker, scale search (opt-in; the entries above are untouched by it): the box follows a face that grows or
 * shrinks, one level a frame.  tests/track_scale_restatement.py restates it; DESIGN.md section 4 holds the specification.
 * All integers, / is the floor.
 * Levels: the seed's template is tw0 x th0, L0 = max(tw0, th0); level L has tw(L) = (tw0 L + L0 / 2) / L0 and th(L) likewise
 * (one level is one sample on the longer side); L is valid when 4 <= tw(L), th(L) <= 64, tw(L) <= gw, th(L) <= gh.  The state:
 * templ, the template T0, always tw0 x th0, packed as above; pos int32[3] = (x, y, L), (x, y) the corner of the box at L's size.
 * resample(A, n_in -> n_out) per axis, bilinear at pixel centres, 6-bit weights: num = (2 i + 1) n_in - n_out, den = 2 n_out;
 * num < 0: i0 = 0, f = 0, else i0 = num / den, f = ((num - i0 den) 64) / den; i1 = min(i0 + 1, n_in - 1), i0 = min(i0, n_in - 1);
 * v = (A[y0][x0] (64 - fy)(64 - fx) + A[y0][x1] (64 - fy) fx + A[y1][x0] fy (64 - fx) + A[y1][x1] fy fx + 2048) >> 12.
 * d3f_track_seed_scale_u8: d3f_track_seed_u8 with pos int32[3], pos[2] = L0 (one launch, the same kernel).
 * d3f_track_search_scale_u8: gray [B][gh][gw]; templ and pos read at the start and written at the end (a level outside the
 * valid ones, then a position outside the image, is moved inside first).  For each frame in order:
 *   - candidate levels Lc = L + dL, dL in -levels..levels, the invalid ones dropped; T(Lc) = resample(T0 -> th(Lc) x tw(Lc));
 *     the anchor keeps the centre, ax = x + (tw(L) - tw(Lc)) / 2 clamped into 0..gw - tw(Lc), ay likewise;
 *   - candidates (dx, dy) in [-search, search]^2 with the box at (ax + dx, ay + dy) inside the image;
 *   - cost = sum |gray - T(Lc)| over the box, ncost = (cost << 12) / (tw(Lc) th(Lc)) (1/4096 grey levels per sample);
 *   - the smallest (ncost + penalty |dL|, |dL|, dL + 1, dx dx + dy dy, dy + search, dx + search) wins: fields of 21, 1, 2, 14, 8
 *     and 8 bits of one unsigned 64-bit key.  Ties go to no change of size, then to shrinking, then as above;
 *   - found = cost <= lost tw(Lc) th(Lc), on the winner's own cost.  Found: L = Lc, (x, y) = anchor + (dx, dy),
 *     W0 = resample(the window at the new box -> th0 x tw0), T0 = (T0 (8 - adapt) + W0 adapt + 4) >> 3.  Not found: x, y, L and
 *     T0 stay exactly as they were;
 *   - out[b] = (x, y, tw(L), th(L), ncost, found, L, cost), int32[8], after the update.
 * levels is 0 (the search of d3f_track_search_u8: the same positions, costs and template) or 1; penalty, in 1/4096 grey
 * levels, 0..65535, is hysteresis against size jitter on flat content (D3F_TRACK_SCALE_PENALTY, an eighth of a level: a
 * design choice, not a measurement).  The stride is fixed at the seed, so the longer side can grow to 64 samples and shrink
 * to 4; beyond that the level stays at its limit, and another key box seeds at a new stride.
 * Back in the frame, with the seed's geometry: fw' = (fw L + L0 / 2) / L0, x' = ((2 x + tw(L)) s + 2 ox + fw - tw0 s - fw') / 2,
 * fh' and y' likewise (ops.track_scale_faces); at L0 that is (x s + ox, y s + oy, fw, fh).
 * d3f_track_template_scale_u8: d3f_gray_decimate_u8 into gray_ws, then d3f_track_search_scale_u8: two launches in one call.
 * B == 0 touches nothing.  Refused before any device call: what the entries above refuse, levels outside 0..1, penalty
 * outside 0..65535. */
#define D3F_TRACK_SCALE_PENALTY 512
int d3f_track_seed_scale_u8(const uint8_t* frame, int h, int w, int s, int tx, int ty, int tw, int th, uint8_t* templ,
                            int32_t* pos, void* stream);
int d3f_track_search_scale_u8(const uint8_t* gray, int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost,
                              int levels, int penalty, uint8_t* templ, int32_t* pos /* int32[3]: x, y, L */,
                              int32_t* out /* [B][8] */, void* stream);
int d3f_track_template_scale_u8(const uint8_t* frames, int B, int h, int w, int s, int tw0, int th0, int search, int adapt,
                                int lost, int levels, int penalty, uint8_t* templ, int32_t* pos, uint8_t* gray_ws,
                                int32_t* out, void* stream);

/* Template tracker, rotation search (opt-in; the entries above are untouched by it): the box follows head roll, one angle
 * index a frame, and writes the angle that the _rboxes_ operators read.  tests/track_rot_restatement.py restates it; DESIGN.md
 * section 4 holds the specification.  All integers, / is the floor, >> of a negative number too.  It does not search the size.
 * The state: templ, the template T0 of the UPRIGHT face, tw0 x th0, packed as above; pos int32[3] = (x, y, a): (x, y) the corner
 * of the un-rotated tw0 x th0 box, which turns about its centre as the _rboxes_ boxes do, a the angle index in -amax..amax.
 * Index a is the angle a * step hundredths of a degree; step is the host's choice (D3F_TRACK_ROT_STEP = 200, D3F_TRACK_ROT_MAX =
 * 60 degrees).  table: HOST memory, int32 [2 amax + 1][2], entry a + amax = (c16, s16) = round(65536 cos), round(65536 sin) of
 * that angle (ops.box_rotation; x right, y down, positive clockwise on the screen); amax <= D3F_TRACK_ROT_MAX_INDEX.  The table
 * is checked (every entry within -65536..65536) and passed by value; the device does no trigonometry.
 * The disc: with u = 2 i + 1 - tw0, v = 2 j + 1 - th0, D = min(tw0, th0), sample (i, j) belongs when u u + v v <= D D; n is
 * their number.  Costs are summed and T0 is blended on the disc only.
 * rot(A, c, s), A of th0 x tw0, per sample of the disc: X = c u + s v + (tw0 - 1) 65536, Y = -s u + c v + (th0 - 1) 65536 (units
 * of 1/131072 sample); x0 = X >> 17, fx = (X >> 11) & 63, x1 = x0 + 1, both clamped to 0..tw0 - 1, y likewise; the value is the
 * scale search's bilinear form, (A[y0][x0] (64 - fy)(64 - fx) + ... + 2048) >> 12.  At angle 0 it is the identity.  (A tap of a
 * sample on the disc's rim may be a sample just outside the disc.)
 * d3f_track_seed_rot_u8: d3f_track_seed_u8's launch, then one more: on the disc templ = rot(the grey, c16, -s16), the key box's
 * content turned back by the key angle, and pos[2] = a0.  With a0 = 0, c16 = 65536, s16 = 0 templ is the plain seed's bytes.
 * d3f_track_search_rot_u8: gray [B][gh][gw]; templ and pos read at the start and written at the end (an a outside -amax..amax
 * and a position outside the image are moved inside first).  For each frame in order:
 *   - candidate indices a + dA, dA in -steps..steps, those outside -amax..amax dropped; T(a + dA) = rot(T0, c, s) of the index;
 *   - candidates (dx, dy) in [-search, search]^2 with the un-rotated box inside the image, as d3f_track_search_u8 has them;
 *   - cost = sum over the disc of |gray - T(a + dA)|, ncost = (cost << 12) / n;
 *   - the smallest (ncost + penalty |dA|, |dA|, dA + 1, dx dx + dy dy, dy + search, dx + search) wins: the scale search's 64-bit
 *     key with dA in the place of dL.  Ties go to no turn, then to the smaller index, then as above;
 *   - found = cost <= lost n, on the winner's own cost.  Found: a += dA, (x, y) += (dx, dy), W0 = rot(the window at the new box,
 *     c, -s) of the new index, T0 = (T0 (8 - adapt) + W0 adapt + 4) >> 3 on the disc.  Not found: x, y, a and T0 stay;
 *   - out[b] = (x, y, tw0, th0, ncost, found, a, cost), int32[8], after the update.
 * The box in the frame is d3f_track_search_u8's, (x s + ox, y s + oy, fw, fh); its angle is a * step hundredths of a degree.
 * d3f_track_template_rot_u8: d3f_gray_decimate_u8 into gray_ws, then d3f_track_search_rot_u8: two launches in one call.
 * B == 0 touches nothing.  Refused before any device call: what d3f_track_search_u8 refuses, steps outside 0..1, penalty outside
 * 0..65535, amax outside 0..D3F_TRACK_ROT_MAX_INDEX, a null table or an entry outside -65536..65536; by the seed an a0 outside
 * -D3F_TRACK_ROT_MAX_INDEX..D3F_TRACK_ROT_MAX_INDEX and c16, s16 outside -65536..65536. */
#define D3F_TRACK_ROT_MAX_INDEX 64
#define D3F_TRACK_ROT_STEP 200
#define D3F_TRACK_ROT_MAX 60
#define D3F_TRACK_ROT_PENALTY 512
int d3f_track_seed_rot_u8(const uint8_t* frame, int h, int w, int s, int tx, int ty, int tw, int th, int a0, int c16, int s16,
                          uint8_t* templ, int32_t* pos /* int32[3]: x, y, a */, void* stream);
int d3f_track_search_rot_u8(const uint8_t* gray, int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost,
                            int steps, int penalty, int amax, const int32_t* table /* host [2 amax + 1][2] */, uint8_t* templ,
                            int32_t* pos /* int32[3]: x, y, a */, int32_t* out /* [B][8] */, void* stream);
int d3f_track_template_rot_u8(const uint8_t* frames, int B, int h, int w, int s, int tw0, int th0, int search, int adapt,
                              int lost, int steps, int penalty, int amax, const int32_t* table, uint8_t* templ, int32_t* pos,
                              uint8_t* gray_ws, int32_t* out, void* stream);

/* Template tracker, re-acquisition (opt-in; the entries above are untouched by it): a face that the search window loses --
 * it left the frame and came back elsewhere, a cut away and back, a hand in front of it -- is looked for in the whole
 * frame.  tests/track_reacq_restatement.py restates it; DESIGN.md section 4 holds the specification.  All integers, unsigned
 * where a key is formed.  It searches neither the size nor the angle: the state is the plain entries'.
 * The key template K (key_templ: packed as templ is, tw bytes a row, th rows) holds the bytes the seed wrote into templ; it is
 * never adapted and never written by these entries, and the next seed replaces it.  An adapted template drifts; the key box
 * was marked by hand.
 * d3f_track_global_u8: gray [B][gh][gw], any byte address; per frame b, independent of every other frame and of the tracker's
 * state:
 *   - every position (x, y) with 0 <= x <= gw - tw and 0 <= y <= gh - th is a candidate;
 *   - cost = sum over the template of |gray[b][y + j][x + i] - K[j][i]|, below 2^20;
 *   - key = cost << 32 | y << 16 | x, unsigned 64 bits (sizes are at most 16384: each coordinate fits its field);
 *   - keys[b] = the smallest key: equal costs go to the top-most position, then the left-most; a constant image gives
 *     (cost, 0, 0).  A minimum: exact in any order of evaluation.
 * Two launches: keys[0..B) set to all-ones, then a grid of (tiles of 16 x 8 candidate positions, B) workgroups, each taking
 * its tile's smallest key into keys[b] with one 64-bit atomicMin (an ordinary vector atomic).  No dword is loaded whole
 * outside gray's B gh gw bytes, and nothing outside keys[0..B) is written.
 * d3f_track_search_reacq_u8: d3f_track_search_u8 with keys [B] of the same gray and K.  For each frame in order:
 *   - the step of d3f_track_search_u8 exactly as it is.  Found: pos and templ are updated as there, out[b] = (x, y, cost, 1);
 *   - not found: gcost = keys[b] >> 32.  gcost <= relost * tw * th: pos = (keys[b] & 0xffff, (keys[b] >> 16) & 0xffff), templ = K
 *     byte for byte, out[b] = (pos.x, pos.y, gcost, 2).  Otherwise pos and templ stay, out[b] = (pos.x, pos.y, cost, 0) as there;
 *   - the next frame searches its window from wherever this one ended.
 * keys[b] depends on frame b and K alone, so cutting a call anywhere changes nothing.  relost, 0..255 grey levels a sample:
 * D3F_TRACK_RELOST = 8, half of D3F_TRACK_LOST -- a whole frame has tens of thousands of candidates where the window has a
 * thousand, so it gets the stricter threshold: a design choice, not a measurement (on the tests' recipe K costs 2.4 .. 2.9
 * levels a sample where the patch is and 30 .. 33 at the best place of a frame without it).  relost = 0 re-acquires only an
 * exact copy of K.
 * d3f_track_template_reacq_u8: d3f_gray_decimate_u8 of the frames into gray_ws [B][gh][gw], d3f_track_global_u8 of it into
 * keys_ws [B], then d3f_track_search_reacq_u8: four launches in one call.
 * B == 0 touches nothing.  Refused before any device call: what d3f_track_search_u8 refuses (d3f_track_global_u8: of that, what
 * it has arguments for), relost outside 0..255, a null key_templ or keys, keys not 8-byte aligned, key_templ overlapping templ
 * (the tw * th bytes of each). */
#define D3F_TRACK_RELOST 8
int d3f_track_global_u8(const uint8_t* gray, int B, int gh, int gw, int tw, int th, const uint8_t* key_templ,
                        uint64_t* keys /* uint64 [B] */, void* stream);
int d3f_track_search_reacq_u8(const uint8_t* gray, int B, int gh, int gw, int tw, int th, int search, int adapt, int lost,
                              int relost, uint8_t* templ, const uint8_t* key_templ, int32_t* pos, const uint64_t* keys,
                              int32_t* out /* [B][4] */, void* stream);
int d3f_track_template_reacq_u8(const uint8_t* frames, int B, int h, int w, int s, int tw, int th, int search, int adapt,
                                int lost, int relost, uint8_t* templ, const uint8_t* key_templ, int32_t* pos, uint8_t* gray_ws,
                                uint64_t* keys_ws, int32_t* out, void* stream);

/* log_batch_as_image_grid of the three LitModules (d3f/train_deep_fake/lit_module.py:235-249,
 * d3f/train_denoiser/lit_module.py:157-171, d3f/balance_training_images/lit_module.py:197-211):
 * torchvision.utils.make_grid(batch[:images], nrow, padding, pad_value), the whole grid -- padding included -- taken
 * through * scale + shift and clamp(0, 1), then TensorBoard's uint8 conversion (* 255, truncated), as HWC bytes.
 * Layout: xmaps = min(nrow, images), ymaps = ceil(images / xmaps); the grid is GH x GW = (ymaps * (H + padding) + padding)
 * x (xmaps * (W + padding) + padding); image k at row (k / xmaps) * (H + padding) + padding, column (k % xmaps) *
 * (W + padding) + padding; everything else, the blank cells of a ragged last row too, is pad_value; images == 1 gives the
 * bare H x W image; C == 1 is replicated to three channels.  Value: t = v * scale + shift in fp32 (product and sum
 * rounded separately), t = fminf(fmaxf(t, 0), 1) (NaN -> 0), byte = (uint8_t)(t * 255.0f).
 * d3f_image_grid_shape (host only) writes {GH, GW}.  d3f_image_grid_u8: batches is a HOST array of n device pointers to
 * fp32 NCHW batches [B][C][H][W] of one shape; out [n][GH][GW][3] (any byte alignment); one launch for all n.
 * Refused before any device call: n outside 1..8, images outside 1..B, nrow < 1, padding outside 0..64, H or W outside
 * 1..16384, C other than 1 or 3, an output of 2^31 bytes or more, null pointers. */
int d3f_image_grid_shape(int images, int nrow, int padding, int H, int W, int32_t dims[2]);
int d3f_image_grid_u8(const float* const* batches, int n, int B, int C, int H, int W, int images, int nrow, int padding,
                      float pad_value, float scale, float shift, uint8_t* out, void* stream);

/* GPU-side augmentation of the training step (d3f/train_denoiser/lit_module.py:55-65 RandomAffine, applied at :113):
 * out[b] = grid_sample(in[b], affine_grid(theta[b]), bilinear, zeros padding, align_corners=False), NCHW f32,
 * theta [B][2][3] row-major (normalised output -> input coordinates).  in and out must not alias. */
int d3f_affine_warp(const float* in, const float* theta, float* out, int B, int C, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------
 * Counter-based random numbers (Philox4x32-10, Random123 / cuRAND definition) made inside the kernels that consume
 * them.  The draw layout every entry below shares:
 *   key     = (seed & 0xffffffff, seed >> 32)                    seed, offset: caller-given uint64
 *   counter = (g, b, offset & 0xffffffff, offset >> 32)          b: image index inside the call
 *   normals  g = index of a group of four consecutive elements of image b (per_image % 4 == 0, per_image / 4 < 0xFFFFFFFD);
 *            words x0..x3: ua = ((x0 >> 9) + 0.5) * 2^-23, ub = (x1 >> 8) * 2^-24, R = sqrt(-2 ln ua),
 *            z0 = R cos(2 pi ub), z1 = R sin(2 pi ub); x2, x3 give z2, z3 the same way (fp32, accurate ln / sqrt / sincospi)
 *   y        word 0 of g = 0xFFFFFFFF: y = (x0 >> 8) * 2^-24 in [0,1)
 *   u0..u3   the four words of g = 0xFFFFFFFE, u4 = word 0 of g = 0xFFFFFFFD (augmentation; same conversion as y)
 * A value depends on (seed, offset, b, element) only: not on B, the grid, or per_image beyond the element's own index.
 * Every consumer has a twin that writes out exactly the draws it uses, from the same device functions.
 * ------------------------------------------------------------------------------------- */
/* host: one Philox4x32-10 block (tests, tools; no device needed) */
int d3f_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);

/* GPU-side augmentation with its parameters drawn inside: replaces the draws + theta + warp (+ where) of RandomAffine
 * (d3f/train_denoiser/lit_module.py:55-65, applied at :113; kind 0, params = degrees, translate_x, translate_y, scale_lo,
 * scale_hi; always applied) and of A.ShiftScaleRotate (d3f/train_deep_fake/lit_module.py:99-111; kind 1, params =
 * shift_limit, scale_limit, rotate_limit, p, unused).  Draw layout above: u0..u3 of image b from g = 0xFFFFFFFE, u4 from
 * g = 0xFFFFFFFD.
 *   kind 0: ang = (2 u0 - 1) radians(degrees), sc = u1 (scale_hi - scale_lo) + scale_lo, tx = (2 u2 - 1) translate_x 2,
 *           ty = (2 u3 - 1) translate_y 2;  theta = [[cos/sc, -sin/sc, tx], [sin/sc, cos/sc, ty]]
 *   kind 1: angle = (2 u0 - 1) rotate_limit (degrees), scale = 1 + (2 u1 - 1) scale_limit, dx = (2 u2 - 1) shift_limit,
 *           dy = (2 u3 - 1) shift_limit, apply = u4 < p;  theta of cv2.warpAffine(getRotationMatrix2D(centre, angle, scale)
 *           + (dx W, dy H)) in affine_grid form
 * then the sampling of d3f_affine_warp.  An image whose `apply` draw fails passes through as a copy.  in and out must
 * not alias. */
int d3f_affine_warp_rng(const float* in, float* out, uint64_t seed, uint64_t offset, int kind,
                        const float params[5], int B, int C, int H, int W, void* stream);
/* the theta [B][2][3] and apply [B] (uint8) that call uses (same layout, same device functions) */
int d3f_affine_theta_draw(uint64_t seed, uint64_t offset, int kind, const float params[5],
                          float* theta, uint8_t* apply, int B, int H, int W, void* stream);

/* Device dataset: a training batch assembled from a pool of decoded images that stays in device memory.  Replaces, per
 * step, the host's decode + transform (d3f/dataset/image_dataset.py:33-44), the copy of the batch to the device, and the
 * augmentation of d3f/train_deep_fake/lit_module.py:99-111 (A.Normalize + A.ShiftScaleRotate) or of
 * d3f/train_denoiser/lit_module.py:55-65,113 (RandomAffine) -- one launch.
 *   pool [N][H][W][3] uint8 RGB (the input layout of d3f_u8rgb_normalise), index [B] int64 on the device,
 *   out [B][3][H][W] f32, mean / std host arrays.
 *   plain (theta == NULL, apply == NULL): out[b] = ((float)pool[index[b]] / 255 - mean[c]) / std[c], the bits of
 *     d3f_u8rgb_normalise;
 *   theta [B][2][3]: the plain image through the sampling of d3f_affine_warp where apply[b] != 0 (apply [B] uint8 on the
 *     device; NULL: every image), the plain image elsewhere -- the bits of torch.where(apply, warp(x, theta), x);
 *   d3f_pool_batch_rng: the plain image through d3f_affine_warp_rng(seed, offset, kind, params): same draw layout, an
 *     image whose `apply` draw fails is the plain image.
 * The three forms and the two warp entries above instantiate ONE sampling function and ONE theta function; with
 * contraction off the fused result is bit for bit the composition it replaces.
 * An index outside [0, N) makes that output image all NaN; nothing is read for it, the other images are unaffected.
 * Image bases are 64-bit (N * H * W * 3 may pass 2^32) and need no alignment.
 * Refused before any device call: a null pool / index / out / mean / std / params (index and out may be null at B == 0,
 * which launches nothing), N < 1, B < 0, H or W < 1, a zero std, an image of 2^31 bytes or more, apply without theta, a bad
 * kind or bad params (as d3f_affine_warp_rng). */
int d3f_pool_batch(const uint8_t* pool, int64_t N, const int64_t* index, float* out, int B, int H, int W,
                   const float mean[3], const float std[3], const float* theta, const uint8_t* apply, void* stream);
int d3f_pool_batch_rng(const uint8_t* pool, int64_t N, const int64_t* index, float* out, int B, int H, int W,
                       const float mean[3], const float std[3], uint64_t seed, uint64_t offset, int kind,
                       const float params[5], void* stream);

/* Balanced sampling: d3f_pool_batch_rng with the index of every image drawn inside the launch, from the difficulty classes
 * `d3f balance` writes.  The table lies in device memory:
 *   members [M] int64: the listed images, sorted by (class, index);
 *   class_start [Kn + 1] int64: offsets into members of the Kn classes that have an image (empty classes are left out).
 * Image b of the stream (seed, offset) is, with x = block 0xFFFFFFFD of image b (word 0 is the augmentation's Bernoulli
 * draw):  j = (x1 * Kn) >> 32,  cnt = class_start[j + 1] - class_start[j],  m = (x2 * cnt) >> 32,
 *         index = members[class_start[j] + m]        (64-bit products of 32-bit words)
 * -- every class with equal probability, every image of a class with equal probability, with replacement; a function of
 * (seed, offset, b) alone.  index_out [B] int64 receives the indices; out is d3f_pool_batch_rng(pool, N, index_out, ...),
 * bit for bit.  kind: 0 / 1 as d3f_affine_warp_rng, or D3F_AUGMENT_NONE (params may be NULL): the plain image.
 * d3f_balanced_index_draw writes the same indices without touching a pool.
 * Refused before any device call: what d3f_pool_batch_rng refuses, a null members / class_start / index_out (index_out and
 * out may be null at B == 0, which launches nothing), Kn < 1, B > 65535. */
#define D3F_AUGMENT_NONE (-1)
int d3f_pool_batch_balanced_rng(const uint8_t* pool, int64_t N, const int64_t* members, const int64_t* class_start, int Kn,
                                float* out, int64_t* index_out, int B, int H, int W, const float mean[3],
                                const float std[3], uint64_t seed, uint64_t offset, int kind, const float params[5],
                                void* stream);
int d3f_balanced_index_draw(const int64_t* members, const int64_t* class_start, int Kn, uint64_t seed, uint64_t offset,
                            int64_t* index_out, int B, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training-step arithmetic around the network
 * ------------------------------------------------------------------------------------- */
/* blend_random_amount_of_noise_with_each_sample + sample_random_number_from_exponential_distribution
 * (d3f/train_denoiser/lit_module.py:128-153 == d3f/train_deep_fake/lit_module.py:208-233) given the
 * caller's draws noise ~ N(0,1) [B][per_image] and y ~ U[0,1) [B]:
 *   r = (1/lam) * log(1 / (y*(1-c) + c)), c = exp(-lam);  out = sqrt(1-r)*x + sqrt(r)*noise */
int d3f_noise_blend(const float* x, const float* noise, const float* y_uniform, float lam, float* out,
                    float* r_out_or_null, int B, int64_t per_image, void* stream);
/* blend_fixed_amount_of_noise_with_each_sample (d3f/balance_training_images/lit_module.py:109-121) given the
 * caller's noise and the per-image ratios r [B] (device): out = sqrt(1-r)*x + sqrt(r)*noise */
int d3f_noise_blend_fixed(const float* x, const float* noise, const float* r, float* out, int B, int64_t per_image,
                          void* stream);
/* d3f_noise_blend with z and y drawn inside, K12 as one kernel (d3f/train_denoiser/lit_module.py:128-153 ==
 * d3f/train_deep_fake/lit_module.py:208-233: randn_like + rand + blend): out = sqrt(1-r) x + sqrt(r) z.  Draw layout above:
 * the four normals of elements 4g .. 4g+3 of image b from counter g, y from g = 0xFFFFFFFF.  Given the same z and y the
 * result is d3f_noise_blend's bit for bit.  out must not alias x (the callers never do). */
int d3f_noise_blend_rng(const float* x, uint64_t seed, uint64_t offset, float lam, float* out,
                        float* r_out_or_null, int B, int64_t per_image, void* stream);
/* d3f_noise_blend_fixed with z drawn inside (d3f/balance_training_images/lit_module.py:109-121): fixed ratios r [B] on
 * the device; normals as above, no y.  out must not alias x. */
int d3f_noise_blend_fixed_rng(const float* x, uint64_t seed, uint64_t offset, const float* r, float* out, int B,
                              int64_t per_image, void* stream);
/* d3f_noise_blend_fixed_rng with the Philox counter's image word taken from index[b] instead of b (held-out validation:
 * an image meets the same noise every epoch, whatever batch it arrives in and wherever in it).  index [B] int64 on the
 * device.  With index = 0 .. B-1 the output equals d3f_noise_blend_fixed_rng's bit for bit; the draw layout is otherwise
 * unchanged.  The index lives on the device, so this entry cannot refuse a value outside [0, 2^32): such an image names no
 * counter and is written as NaN (every element), which no later score can hide.  out must not alias x. */
int d3f_noise_blend_fixed_index_rng(const float* x, uint64_t seed, uint64_t offset, const float* r, const int64_t* index,
                                    float* out, int B, int64_t per_image, void* stream);
/* the draws of the calls above, written out: noise [B][per_image] (normals of counter g = element / 4), y [B]
 * (g = 0xFFFFFFFF); either may be NULL */
int d3f_noise_draw(uint64_t seed, uint64_t offset, float* noise_or_null, float* y_or_null, int B, int64_t per_image,
                   void* stream);
/* compute_difficulty_loss (d3f/balance_training_images/lit_module.py:139-142): out[b] = mean |prediction - target|
 * over image b; deterministic two-pass sum (f64 partials in the workspace) */
size_t d3f_l1_per_image_workspace_bytes(int B);
int d3f_l1_per_image(const float* prediction, const float* target, float* out, void* workspace, int B,
                     int64_t per_image, void* stream);
/* The scoring epoch of balance_training_images on the device (csrc/difficulty.hip).
 *
 * d3f_l1_per_image_scatter -- compute_difficulty_loss (d3f/balance_training_images/lit_module.py:137-140) written where
 * validation_step's `index` says (:122-135): scores[index[b]] = d3f_l1_per_image's out[b], bit for bit (the same partial
 * stage, the same last-stage expression).  index [B] int64 and scores [N] fp32 on the device; an index outside [0, N)
 * writes nothing; two equal indices in one call leave either value; entries no index names are not touched.  B == 0
 * launches nothing.  workspace: d3f_l1_per_image_workspace_bytes(B). */
int d3f_l1_per_image_scatter(const float* prediction, const float* target, const int64_t* index, float* scores, int N,
                             void* workspace, int B, int64_t per_image, void* stream);
/* compute_difficulty_index_for_each_loss (d3f/balance_training_images/lit_module.py:181-193) over a score buffer in which
 * NaN means "not scored": such an entry gets class -1 and takes no part in min, max or the counts.  A scored entry s:
 *   q = (s - min) / (max - min)      one IEEE fp32 subtraction and one IEEE fp32 division (no reciprocal, no contraction)
 *   q = min(max(q, 0.f), 0.99999f)   (:189)
 *   class = (int64)(q * (float)number_of_classes), truncated   (:191)
 * DIFFERENCE from the reference, on purpose: when max == min (every scored entry equal, or a single one) the reference
 * divides 0 by 0 and `.long()` of the NaN is INT64_MIN; here every scored entry gets class 0.
 * classes [N] int64; counts [number_of_classes] int32 = scored entries per class (integer adds: independent of the launch
 * geometry); minmax [2] fp32 = {min, max}, NaN twice when nothing was scored.  number_of_classes 1..65536.  N == 0: no
 * kernel, counts zeroed, minmax NaN.  workspace: d3f_difficulty_classes_workspace_bytes(N). */
size_t d3f_difficulty_classes_workspace_bytes(int N);
int d3f_difficulty_classes(const float* scores, int N, int number_of_classes, int64_t* classes, int32_t* counts,
                           float* minmax, void* workspace, void* stream);
/* The figure validation_epoch_end logs as `difficulty_class_histogram` (d3f/balance_training_images/lit_module.py:151-155:
 * axes.hist(difficulty_index), matplotlib's default of 10 bins): the counts and a chart of them, without a host round trip
 * in between.  classes [N] int64 on the device; entries < 0 are passed over.
 * Counts: numpy.histogram(x, bins) over the entries >= 0.  lo, hi = min, max (0, 1 without data); lo == hi: lo -= 0.5,
 * hi += 0.5; edges e_k = k * ((hi - lo) / bins) + lo in float64, e_bins = hi; an entry counts for the k with
 * e_k <= v < e_(k+1), the last bin closed.  bin_counts [bins] int32, range [2] float64 = {lo, hi}.
 * Chart: uint8 [H][W][3], integer geometry (every division truncates): background 255; box x0 = W/8, x1 = W - W/10,
 * y0 = H*3/25, y1 = H - H*11/100; frame colour 0 on rows y0 and y1-1 over [x0, x1) and columns x0 and x1-1 over [y0, y1);
 * interior xi0 = x0+1, xi1 = x1-1, yi0 = y0+1, yi1 = y1-1, IW = xi1-xi0, IH = yi1-yi0; bar i covers the columns
 * [xi0 + i*IW/bins, xi0 + (i+1)*IW/bins) and the rows [yi1 - h_i, yi1), h_i = counts[i]*IH*20 / (cmax*21) in 64-bit
 * integers (0 when the largest count cmax is 0; the tallest bar ends at 1/1.05 of the box like matplotlib's y margin),
 * colour (31, 119, 180).  No text, no ticks.  Refused before any device call: bins < 1, bins > IW, H or W outside
 * 32..16384, null pointers.  workspace: d3f_difficulty_histogram_u8_workspace_bytes(N). */
size_t d3f_difficulty_histogram_u8_workspace_bytes(int N);
int d3f_difficulty_histogram_u8(const int64_t* classes, int N, int bins, int32_t* bin_counts, double* range, uint8_t* chart,
                                int H, int W, void* workspace, void* stream);
/* MseStructuralSimilarityLoss(input_min, input_max)(prediction, target)
 * (d3f/loss_functions/structural_similarity_loss.py:14-26; piqa.SSIM defaults) on NCHW f32
 * [B][3][H][W]: loss_out = {loss, mse, ssim}; grad_pred = d loss / d prediction. */
size_t d3f_mse_ssim_loss_workspace_bytes(int B, int H, int W);
int d3f_mse_ssim_loss(const float* pred, const float* target, float input_min, float input_max,
                      float* loss_out, float* grad_pred, void* workspace, int B, int H, int W, void* stream);
/* The criterion's terms per image, forward only (csrc/quality.hip): what a held-out validation pass scores.
 * MseStructuralSimilarityLoss (d3f/loss_functions/structural_similarity_loss.py:14-26; piqa.SSIM defaults) restricted to
 * image b of NCHW f32 [B][3][H][W] inputs:
 *   mse  = mean over its 3*H*W raw elements of (p - t)^2
 *   ssim = mean over its 3*(H-10)*(W-10) valid positions of the SSIM map (d3f_mse_ssim_loss's arithmetic: the same
 *          normalisation, fp32 taps, column-then-row order, tap order and constants; no fused multiply-add)
 *   loss = (mse + (1.0f - ssim)) / 2.0f
 *   psnr = -10 log10(mse01), mse01 = mean of (norm01(p) - norm01(t))^2 (norm01: to [0, 1] by the input range, clipped);
 *          +inf when mse01 is 0
 * metrics [4][N] f32 on the device, rows mse, ssim, psnr, loss; image b's values go to column index[b] (int64, device), or
 * to column b when index is NULL.  As d3f_l1_per_image_scatter: an index outside [0, N) writes nothing, entries no index
 * names are not touched, B == 0 launches nothing.  One stencil pass and a float64 sum of each image's tile partials in a
 * fixed order: an image's four values have the same bits whatever batch it is scored in and wherever in it, and a repeat
 * is bit for bit.  Refused on the host before any device call: null pointers (index apart), H or W below 11,
 * input_max <= input_min, N < 1, more than 21845 images.  workspace: d3f_quality_per_image_workspace_bytes(B, H, W). */
size_t d3f_quality_per_image_workspace_bytes(int B, int H, int W);
int d3f_quality_per_image_scatter(const float* prediction, const float* target, float input_min, float input_max,
                                  const int64_t* index_or_null, float* metrics, int N, void* workspace, int B, int H, int W,
                                  void* stream);
/* torch.optim.Adam step over a flat buffer (lit_module.py:95 / train_deep_fake/lit_module.py:116-120);
 * step counts from 1; grad_scale multiplies the gradient first (1/world_size for data parallel) */
int d3f_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* stream);
/* ema.lerp_(online, weight)  (ema_pytorch update used at d3f/train_deep_fake/lit_module.py:185) */
int d3f_ema_lerp(float* ema, const float* online, int64_t n, float weight, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* D3F_HIP_H */
