/* scot_plan.h — running, EVALUATING and fine-tuning a trained ScOT model from C: exported inference plans, their adjoints, training
 * plans, on one stream or two, and the error sums of a prediction or a whole rollout (ABI 8).
 *
 * scot_hip.h is the kernel-level boundary: about a hundred entry points that a host program has to order itself.  This header is the
 * model-level one.  `ScOT.export_plan` (poseidon_amd/plan.py) records one inference forward for one input signature and writes it,
 * with the weights, as a relocatable plan image; the calls below load such a file and run it.  A host needs nothing but the
 * shared library and the HIP runtime: no Python, no torch.  The prediction is bit-identical to `model(...)` in Python.
 *
 * What a plan covers: the engine's inference forward on ONE stream (or two: TWO-STREAM plans below), at config.image_size or — a
 * RESIZED plan, below — at any square resolution the export was given — no training, no hidden
 * states or attention outputs, no labels (so no pixel_mask INPUT on an inference plan: the mask overwrites the prediction with label
 * values; scot_plan_evaluate_masked takes one beside its targets, a training plan takes one with its batch).  The weights are a
 * snapshot taken at export.  A plan recorded by the binary16 build (libscot_hip_f16.so) loads into that build only; its split-MFMA
 * trunk products run in the bfloat16 build, which the runtime opens from the same directory (or from where the peer call points).
 *
 * An ADJOINT plan (`export_plan(..., adjoint=("pixel_values", "time"))`, image format 2) also covers the frozen model's backward from
 * a cotangent of the prediction to the gradients of these two inputs — what `torch.autograd.grad(output, (pixel_values, time),
 * grad_outputs=g)` returns with every parameter frozen, bit for bit: no labels, no loss, no parameter gradient, no training.  Its
 * forward is the one a differentiable call runs, so beyond an inference plan it holds the saved activations of one forward, the
 * transposed 16-bit weight copy the data gradients read, and room in the gradient arena where a fused layer tail leaves by-products
 * nobody reads.  One vjp per run (the backward reuses saved rows); a rollout leaves nothing to differentiate afterwards, so the
 * adjoint of a whole rollout is a call of its own, scot_plan_rollout_vjp: it recomputes each step from the rollout's predictions.
 *
 * A TRAINING plan (`export_plan(..., labels=..., train=optimizer)`, image format 4; 3 is unassigned) also covers one optimizer step of
 * the fused AdamW the export was given: forward, loss, backward with the weight gradients, update — the Python loop's `zero_grad(overlap=
 * True)`, `model(..., labels=...)`, `loss.backward()`, `opt.step()`.  Its weights are NOT a snapshot: the image holds the fp32 parameters,
 * both 16-bit copies, both moments, the step counters and the gradient scale by value: 4x the fp32 parameter bytes in the 16-bit
 * modes (arena 1x, two moments 2x, two 16-bit copies 1x), 3x in fp32 / bf16x3, plus the small tables.  The runtime owns them after
 * load, scot_plan_run sees the current ones and scot_plan_snapshot writes them back into the image.
 * Weight decay, betas, eps, clipping and the scale schedule are fixed at export; the learning rates are an argument of every step.  Not
 * covered: stochastic depth, partially frozen models, a trimmed image.  Gradient accumulation is covered (section "gradient
 * accumulation" below); data parallelism is composable through scot_plan_gradients and has never been run on more than one GPU.  The reference's
 * pixel_mask is covered: a MASKED training plan (section "pixel masks" below) takes the mask with every batch.  By
 * default it runs on ONE stream, the weight gradients in line (the Python engine puts them on a second stream: measured on
 * Poseidon-B fp16, a plan's step takes 22.7 ms against the Python loop's 19.3 at batch 64, 11.1 against 10.7 at batch 1).
 *
 * A TWO-STREAM plan (`export_plan(..., streams=2)`; image format 5 = an inference plan, 6 = a training plan) holds the engine's own
 * two-stream program instead: the bias tables, the skip blocks, the weight gradients, the gradient fill and the un-scale passes on a
 * SIDE stream beside the main chain, with the engine's fork and join edges as event entries of the image.  The load creates the events
 * and picks a side stream that it MEASURES to run beside the load's stream (scot_stream_overlaps; scot_plan_set_side_stream hands it the
 * host's own instead).  Every call below works on such a plan unchanged and still takes ONE stream: each recorded list forks from it and
 * joins back into it, so runs of one plan stay ordered on the stream you pass.  Results: the prediction is bit-identical to the
 * one-stream plan's; a training step is the engine's two-stream step.  Not covered: adjoint plans (the frozen backward has no
 * weight-gradient stream), more than two streams, and everything a format-4 plan does not cover.  `streams=1` stays the default.
 * Measured on Poseidon-B fp16 with the overlap flag at 1 (profiles/plan_streams/README.md): a training step takes 19.3 ms at batch 64 and
 * 10.5 at batch 1, the Python loop's 19.3 / 10.6, against 22.6 / 11.0 on one stream; inference 6.11 against 6.15 ms at batch 64 — but
 * 3.95 against 3.62 ms at batch 1: for launch-bound inference the event edges cost more than the side stream hides, keep streams=1 there.
 *
 * A RESIZED plan (`export_plan(..., resize=True)` with square inputs of size r != config.image_size; image formats 1, 2 and 5, no new
 * format and no new header word) runs a model at the host's resolution, as the reference's forward does for any input size: its
 * forward list is one scot_spectral_resize call (declared in scot_hip.h) from the input [B, Cin, r, r] to the model's size, the engine's forward, and one
 * scot_spectral_resize from the engine's prediction to [B, Cout, r, r]; the four operator matrices are constants of the image.  An
 * adjoint plan's backward list is the mirror image: the cotangent through the second resize's adjoint, the engine's backward, d_pixel_values
 * through the first one's; d_time is untouched.  H = W = r in scot_plan_describe, and every call below — run, rollout (which resamples
 * at every step, as the reference's rollout does), evaluate, evaluate_masked with element masks at r, vjp, rollout_vjp, poison — works at
 * r unchanged.  Bit-identical to the Python model with `fused_resize = True`.  Not covered: training plans at a foreign resolution
 * (the loss there is not a kernel yet), non-square inputs.  A library from before scot_spectral_resize refuses such an image by the
 * entry point's name (-3).  Measured: profiles/plan_resize/README.md.
 *
 * EVALUATION (every plan; section "evaluation" below).  scot_error_sums is one kernel pair that reduces (prediction, target) to four fp64
 * sums per sample and channel group, and scot_plan_evaluate runs a forward or a whole rollout and leaves ONLY those sums behind: no
 * `steps`-sized prediction buffer, nothing copied to the host.  The sums are what the reference's metrics are made of (its
 * scOT/metrics.py and the compute_metrics of scOT/inference.py): per channel group [slices[g], slices[g+1]) and sample,
 *   S1 = sum |p - t|, N1 = sum |t|, S2 = sum (p - t)^2, N2 = sum t^2        (in this order: sums[..][0..3])
 * and a host turns them into the reference's numbers with a few flops per sample:
 *   lp_error (p = 1, 2)          = Sp^(1/p)
 *   relative_lp_error            = (Sp / Np)^(1/p) * 100 (percent), with Np == 0 replaced by 1e-10
 *   median / mean / std / min / max over the samples (and the means over groups) are the host's job.
 *
 * Status codes as in scot_hip.h: 0, -1 (malformed image / bad argument), -3 (not for this library: ABI, operand format, entry point;
 * or a host other than x86-64 System V, where the replay underneath does not exist), -4 (allocation, copy or launch failed).
 * Runs of ONE plan share its buffers: order them (one stream, or events of the caller's).  Two plans are independent.
 */
#ifndef SCOT_PLAN_H
#define SCOT_PLAN_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#ifndef SCOT_HIP_H
typedef struct ihipStream_t* scot_stream_t; /* = hipStream_t */
#endif
typedef void* scot_plan_t;

/* Validates the WHOLE image first (csrc/plan_image.h: section bounds, counts, every relocation inside its buffer, format version, ABI
 * and operand format equal to this library's, every entry point by name against the library's own list), then allocates the plan's
 * device memory and uploads the constants on `stream`, and waits for the uploads: the image may be released on return.  `image` is
 * host memory, 8-byte aligned.  On failure *plan is NULL and nothing stays allocated. */
int scot_plan_load(const void* image, size_t bytes, scot_plan_t* plan, scot_stream_t stream);
/* out[16]: batch, input channels, H, W, output channels, whether time is an input, its bytes, whether pixel_mask is an input, its
 * bytes, operand format (0 bfloat16, 1 binary16), compute mode (0 fp32, 1 fp16, 2 bf16, 3 bf16x3), bytes of device memory held,
 * recorded calls, bytes of pixel_values, bytes of the prediction, image format version. */
int scot_plan_describe(scot_plan_t plan, long long* out);
/* out[4]: whether the plan resamples (1: a RESIZED plan), the size the model runs at (config.image_size), the size of the host's
 * tensors (H = W above), the number of scot_spectral_resize entries in all its call lists.  Read from the forward list at load. */
int scot_plan_describe_resize(scot_plan_t plan, long long* out);
/* prediction [B, Cout, H, W] <- model(pixel_values [B, Cin, H, W], time [B]); fp32 device buffers of the caller.  time / pixel_mask
 * are NULL exactly when the plan has no such input.  Copies in, replays the recorded calls with every stream slot = `stream` (a
 * two-stream plan: the slots of stream 1 = its side stream), copies out; everything is asynchronous on `stream`. */
int scot_plan_run(scot_plan_t plan, const float* pixel_values, const float* time, const void* pixel_mask, float* prediction,
                  scot_stream_t stream);
/* Autoregressive rollout, the integer form of the reference's (trainer.py:452-603, output_all_steps): time / steps once (rounded as torch
 * rounds it on the GPU: time * (1.0f / steps)), then `steps`
 * forwards; forward k's prediction goes to predictions + k * B * Cout * H * W and back over the first Cout channels of the input, the
 * other input channels stay as given.  Needs a time input and Cout <= Cin.  Reads `time` on the host once (waits for `stream` there). */
int scot_plan_rollout(scot_plan_t plan, const float* pixel_values, const float* time, const void* pixel_mask, float* predictions,
                      int steps, scot_stream_t stream);
/* Releases the plan's memory (the caller orders this after its last run).  NULL is accepted. */
int scot_plan_free(scot_plan_t plan);

/* Name i of the entry points a plan may call (NULL past the end): what can run is what is listed. */
const char* scot_plan_entry_point(int i);
/* Where the bfloat16 build of the library is, for a binary16 plan's trunk products, if it is not `libscot_hip.so` in this library's
 * own directory.  -3 if the file is not that build at this ABI. */
int scot_plan_peer_library(const char* path);
/* Test aid: every scratch buffer and the prediction's own buffer <- byte on `stream`.  With 0xff a run that reads what it did not
 * write first yields NaN. */
int scot_plan_poison(scot_plan_t plan, int byte, scot_stream_t stream);

/* ---- adjoint plans ---- */
/* out[8]: has adjoint, d_pixel_values available, d_time available, recorded backward calls, bytes kept between run and vjp,
 * default gradient scale (export-time value, as an integer power-of-two exponent), 0, 0.  Format-1 plan: all zeros, status 0. */
int scot_plan_describe_adjoint(scot_plan_t plan, long long* out);
/* (d_pixel_values [B, Cin, H, W], d_time [B]) <- J^T d_prediction at the inputs of the LAST scot_plan_run of this plan.  fp32 device
 * buffers of the caller; an output pointer may be NULL (not copied out); asking for one the plan was not exported with: -1.
 * grad_scale: power of two the 16-bit backward runs under (fp16 plans), 0 = the export-time value; must be 0 or 1 for plans whose
 * backward runs unscaled (fp32, bf16, bf16x3).  Needs a completed scot_plan_run since load / poison / rollout / rollout_vjp / the previous vjp:
 * otherwise -1 and nothing is launched.  On a plan without an adjoint (format 1): -3.  Copies the cotangent in, writes {S, 1/S} into the
 * plan's scale state on `stream`, replays the recorded backward, copies the gradients out; asynchronous on `stream`. */
int scot_plan_vjp(scot_plan_t plan, const float* d_prediction, float* d_pixel_values, float* d_time, float grad_scale,
                  scot_stream_t stream);
/* The adjoint of scot_plan_rollout with NO detach between the steps: (d_pixel_values [B, Cin, H, W], d_time [B]) <- the gradient of
 * sum_k <d_predictions[k], predictions[k]> with respect to pixel_values and time, through the chain the rollout runs: t_step = time /
 * steps (rounded as the rollout rounds it), step k >= 1 reads cat(predictions[k-1], pixel_values[:, Cout:]).
 *   predictions   [steps][B, Cout, H, W]: what scot_plan_rollout wrote for these pixel_values and time (the step inputs; read only)
 *   d_predictions [steps][B, Cout, H, W]: the cotangent of every step's prediction (zeros where a step is not observed)
 * A checkpointed sweep: nothing but the step inputs is kept, and those are the caller's `predictions`.  For k = steps-1 .. 0 the call
 * writes step k's input, replays the forward (which recomputes the saved activations), forms the cotangent d_predictions[k] + the first
 * Cout channels of step k+1's input gradient, writes {S, 1/S} and replays the backward.  COST: `steps` forwards + `steps` backwards per
 * call, on top of the forward rollout that produced `predictions`.  With g_k the input gradient and tau_k the time gradient of step k,
 * in plain fp32 adds in exactly this order (bit for bit what the same chain of single-step gradients gives in Python):
 *   d_pixel_values[:, :Cout] = g_0[:, :Cout]
 *   d_pixel_values[:, Cout:] = ((g_{K-1} + g_{K-2}) + ...) + g_0
 *   d_time                   = (((tau_{K-1} + tau_{K-2}) + ...) + tau_0) * (1 / steps), rounded as the rollout rounds time / steps
 * The sums are formed in the caller's d_pixel_values / d_time; either may be NULL (without a d_pixel_values and with steps > 1 the runtime
 * allocates a carry buffer of that size at the first such call, held until the plan is freed and counted in the described device bytes;
 * -4 if that fails).  Needs no preceding run and leaves none behind: a vjp right after it returns -1.  grad_scale as for the vjp;
 * non-finite values of every step are counted in the grad status.  Reads `time` on the host once (waits for `stream` there).
 * Refused before anything is copied or launched: a plan without an adjoint or without a time input: -3; steps < 1, Cout > Cin, a NULL
 * pixel_values / time / predictions / d_predictions, a grad_scale the vjp refuses, steps > 1 or a d_pixel_values on a plan exported
 * without the pixel_values adjoint, a d_time on a plan exported without the time adjoint: -1. */
int scot_plan_rollout_vjp(scot_plan_t plan, const float* pixel_values, const float* time, const float* predictions,
                          const float* d_predictions, int steps, float* d_pixel_values, float* d_time, float grad_scale,
                          scot_stream_t stream);
/* out[2]: non-finite values the un-scale passes have counted since load (a gradient that overflowed binary16 under the scale arrives
 * as inf / NaN and is counted here, never clipped: run + vjp again under a smaller grad_scale), the scale of the last vjp as an
 * exponent.  Waits for `stream`. */
int scot_plan_grad_status(scot_plan_t plan, long long* out, scot_stream_t stream);
/* Name i of the entry points the BACKWARD of an adjoint plan may call (NULL past the end): the data-gradient chain only — no
 * weight-gradient kernel and no optimizer step is in either list. */
const char* scot_plan_adjoint_entry_point(int i);

/* ---- training plans ---- */
/* out[8]: has training, parameter groups, floats in the parameter arena, recorded calls of one step, bytes of labels, bytes kept
 * between the step's forward and its backward, whether the gradient scale is dynamic (fp16), the kind of the batch's pixel_mask (0 none,
 * 1 channel [B, Cout], 2 element [B, Cout, H, W]).  Format-1/2 plan: all zeros, status 0. */
int scot_plan_describe_training(scot_plan_t plan, long long* out);
/* loss [1] <- what `model(pixel_values, time=time, labels=labels).loss` returns at the plan's CURRENT weights, prediction [B, Cout, H, W]
 * (may be NULL) <- its output.  fp32 device buffers of the caller; labels [B, Cout, H, W].  Replays the step's forward only: no state
 * changes.  Asynchronous on `stream`. */
int scot_plan_loss(scot_plan_t plan, const float* pixel_values, const float* time, const float* labels, float* loss, float* prediction,
                   scot_stream_t stream);
/* One optimizer step on the batch: forward, loss, backward with the weight gradients, AdamW update with the export's clipping.
 * lr is HOST memory, lr[g] for parameter group g in the export's order (the optimizer's param_groups); it is read before the call
 * returns.  loss (device [1], may be NULL) <- the loss BEFORE the update.  Clipping, the skip of a step whose gradient norm is not finite
 * and the fp16 gradient scale are decided on the device: the host learns of them from scot_plan_train_status.  Copies the batch in,
 * replays the three step lists, copies the loss out; asynchronous on `stream`. */
int scot_plan_train_step(scot_plan_t plan, const float* pixel_values, const float* time, const float* labels, const float* lr, float* loss,
                         scot_stream_t stream);
/* out[6]: steps applied, steps skipped, gradient scale (1 where it is not dynamic), the last step's gradient norm before clipping, its
 * clip coefficient, non-finite values the un-scale passes have counted.  Waits for `stream`. */
int scot_plan_train_status(scot_plan_t plan, double* out, scot_stream_t stream);
/* Writes the current value of every state buffer — fp32 parameters, both 16-bit copies, both moments, counters, clip floats, gradient
 * scale — back into `image`: a host copy (`bytes` long) of THE image this plan was loaded from; size, header, buffer table and training
 * words are compared with what was loaded, anything else is -1 with nothing written.  The result is a valid training image that resumes
 * exactly.  Waits for `stream`. */
int scot_plan_snapshot(scot_plan_t plan, void* image, size_t bytes, scot_stream_t stream);
/* Name i of the entry points the three step lists of a training plan may call (NULL past the end).  The weight-gradient kernels and
 * the optimizer are listed here and ONLY here. */
const char* scot_plan_training_entry_point(int i);
/* ---- two-stream plans ---- */
/* *overlaps <- 1 when stream `b` really runs beside stream `a` under the engine's fork / join pattern, 0 when the pair serialises (two
 * streams that share a hardware queue do, silently, as soon as they exchange events) or a == b.  The measurement: one spin kernel of
 * ~0.5 ms on `a`; then K1 on a, an event b waits for, K2 on b beside K3 on a, a second event a waits for — accepted below 2.5 kernel
 * times, the best of two trials.  Waits for both streams; ~4 ms.  For any host that needs a second stream that is worth having: a plan's
 * side stream, the comm stream of the native data-parallel backend.  (The CPU emulation answers 0.) */
int scot_stream_overlaps(scot_stream_t a, scot_stream_t b, int* overlaps);
/* The host's own side stream for a two-stream plan, instead of the one the load picked (which is destroyed): between the load and the
 * first run, otherwise -1; NULL or the load's own stream: -1.  It is measured against the load's stream (scot_plan_describe_streams
 * reports the answer) and used whatever the answer.  The host keeps it alive until the plan is freed.  On a one-stream plan: -3. */
int scot_plan_set_side_stream(scot_plan_t plan, scot_stream_t side);
/* out[4]: streams (1 or 2), events, whether the side stream was measured to run beside the load's stream (0: the plan is correct but
 * its two streams may serialise — the load tried eight candidates and kept the first), whether the side stream is the host's. */
int scot_plan_describe_streams(scot_plan_t plan, long long* out);
/* Test aid, next to scot_plan_poison: later calls issue call list `list` (0 forward, 2 / 3 / 4 the step's forward, backward, update)
 * entry by entry in `order`, a permutation of 0 .. n-1 over the list's n entries (anything else: -1), and synchronise both streams
 * whenever the stream of the next entry differs from the previous one's and at the end: the device executes exactly that order.
 * order = NULL restores the normal replay.  The call does NOT judge whether the order is legal. */
int scot_plan_issue_order(scot_plan_t plan, int list, const int* order, int n);

/* ---- evaluation ---- */
/* Bytes of workspace (device memory) scot_error_sums needs for these arguments; 0 where it would refuse them. */
size_t scot_error_sums_workspace_bytes(int B, int C, int HW, const int* channel_slices, int groups);
/* sums [B][groups][4] (double, device) <- { sum |p - t|, sum |t|, sum (p - t)^2, sum t^2 } over the channels [channel_slices[g],
 * channel_slices[g+1]) and all HW pixels of sample b, of pred and target: fp32 [B, C, HW], contiguous, device memory.  channel_slices is
 * HOST memory: groups + 1 strictly ascending ints in [0, C] (the reference's channel_slice_list), read before the call returns; NULL with
 * groups == 1 is the one group [0, C).  Channels outside every group are not read.  Every term and every sum is fp64 (both values are
 * converted first, then subtracted).  The result is bitwise the same from launch to launch, on any device and at any alignment of the
 * operands: no atomics; each (sample, group) is one contiguous run of floats, cut into chunks of a compile-time constant length, one
 * workgroup per chunk, and a second launch adds a run's partials in chunk order.  Inf and NaN go through: a non-finite input makes exactly
 * the sums it enters non-finite.  workspace: 8-byte aligned device memory of at least the bytes the query above names; its contents on
 * entry do not matter.  Two launches on `stream`, asynchronous.  -1: a NULL pointer, B, C or HW < 1, groups outside 1..32, slices not
 * strictly ascending or outside [0, C], workspace too small (nothing is launched, sums is untouched); -4: a launch failed. */
int scot_error_sums(const float* pred, const float* target, int B, int C, int HW, const int* channel_slices, int groups, double* sums,
                    void* workspace, size_t workspace_bytes, scot_stream_t stream);
/* A forward or a whole rollout that leaves only error sums behind.  channel_slices / groups as above, over the plan's Cout output channels.
 *   steps == 1: exactly the forward of scot_plan_run (time as given, NULL exactly when the plan has no time input); targets [B, Cout, H, W],
 *               sums [B][groups][4].
 *   steps  > 1: exactly the chain of scot_plan_rollout (time / steps with that call's rounding, prediction k copied back over the first Cout
 *               input channels); targets [steps][B, Cout, H, W], sums [steps][B][groups][4].
 * Step k's sums are formed from the plan's own output buffer right after forward k, on `stream` (a two-stream plan: after the list has
 * joined), before that buffer is copied back.  predictions may be NULL: then no prediction leaves the plan and the caller needs no
 * `steps`-sized buffer; if given it receives exactly what scot_plan_rollout (steps == 1: scot_plan_run) writes.  Every image format: on a
 * training plan it replays the inference list at the CURRENT weights (validation between training steps; no state changes); on an adjoint
 * plan it leaves nothing to differentiate, like a rollout: a vjp right after it returns -1.  The kernel's workspace is allocated at the
 * first evaluate call, held until the plan is freed and counted in the described device bytes (-4 if that fails).  Reads `time` on the
 * host once when steps > 1 (waits for `stream` there); everything after that is asynchronous on `stream`.
 * Refused before anything is copied or launched: a NULL pixel_values, targets or sums, steps < 1, groups outside 1..32, slices not strictly
 * ascending or beyond Cout, steps > 1 with Cout > Cin, a time that is NULL where the plan takes one (or given where it takes none): -1;
 * steps > 1 on a plan without a time input, an inference plan with a pixel_mask input: -3. */
int scot_plan_evaluate(scot_plan_t plan, const float* pixel_values, const float* time, const float* targets, int steps,
                       const int* channel_slices, int groups, double* sums, float* predictions, scot_stream_t stream);

/* ---- pixel masks ---- */
/* scot_error_sums of the prediction where(mask, target, pred), in the same pass: what the reference scores after `prediction[pixel_mask]
 * = labels[pixel_mask]` (its scOT/model.py).  mask: device bytes, any non-zero byte = masked, at ANY byte alignment; mask_full == 0: [B, C]
 * (whole planes), mask_full != 0: [B, C, HW].  mask == NULL is exactly scot_error_sums: the same bits, pred untouched.
 *   sums       bit for bit what scot_error_sums returns for where(mask, target, pred): same chunks, same order, no atomics, the same
 *              workspace (scot_error_sums_workspace_bytes).  A masked element enters as if p were t: its term is (double)t - (double)t,
 *              not a literal 0, so an Inf or NaN LABEL under the mask makes the same sums non-finite as in the overwritten tensor; a NaN
 *              or Inf in pred under the mask reaches no sum.
 *   overwrite  != 0: the same pass stores target over pred at the masked positions; every other float of pred keeps its bits.  It needs
 *              groups that tile [0, C) exactly (first slice 0, last slice C), as every channel_slice_list of the reference does: otherwise
 *              -1, nothing is launched, sums and pred are untouched.  == 0: pred is read only.  pred and target may sit at any 4-byte
 *              alignment, as for scot_error_sums (the kernel picks vector or scalar loads per run; the bits are the same).
 * Every other refusal as scot_error_sums. */
int scot_error_sums_masked(float* pred, const float* target, const unsigned char* mask, int mask_full, int overwrite, int B, int C, int HW,
                           const int* channel_slices, int groups, double* sums, void* workspace, size_t workspace_bytes,
                           scot_stream_t stream);
/* scot_plan_evaluate under a pixel_mask: every image format.  pixel_mask is an ARGUMENT of the call, not part of the image: device bytes,
 * [B, Cout] (mask_full == 0) or [B, Cout, H, W] (mask_full != 0), the same mask for all steps.  After forward k, scot_error_sums_masked
 * runs on the plan's own output buffer with overwrite = 1 against targets[k], before that buffer is copied back or out: the sums are the
 * masked sums, the next step's input carries the label values at the masked positions, and `predictions`, if given, receives the
 * overwritten predictions.  pixel_mask == NULL is scot_plan_evaluate, bit for bit.
 * ONE DIFFERENCE FROM THE REFERENCE: its trainer overwrites every rollout step with the FINAL labels; this call uses that step's own
 * target.  The two agree wherever the masked values are constant in time, which holds for every masked channel of the reference's
 * datasets (the constant density and pressure planes, the airfoil's solid cells).
 * Refusals as scot_plan_evaluate, and: a mask with groups that do not tile [0, Cout): -1.  A masked TRAINING plan is not refused for
 * having a mask input (by either evaluate call): the inference list replayed here does not read it. */
int scot_plan_evaluate_masked(scot_plan_t plan, const float* pixel_values, const float* time, const float* targets, const void* pixel_mask,
                              int mask_full, int steps, const int* channel_slices, int groups, double* sums, float* predictions,
                              scot_stream_t stream);
/* MASKED TRAINING PLANS.  `export_plan(pv, time=, labels=, pixel_mask=M, train=opt[, streams=2])` records the step with the mask: bool
 * [B, Cout] is a channel mask (B * Cout bytes), bool [B, Cout, H, W] an element mask (B * Cout * H * W bytes), bool [B, 1, H, W] is
 * expanded over the channels into an element mask; any other shape is refused.  The image (formats 4 and 6, training flag bits 1 and 2)
 * has the mask as one more input buffer; scot_plan_describe reports it and scot_plan_describe_training out[7] its kind (0 none, 1
 * channel, 2 element).  The two calls below are scot_plan_loss / scot_plan_train_step with the batch's mask: device bytes of the plan's
 * mask size.  The loss and the gradients are those of `model(..., labels=, pixel_mask=)`, and the returned prediction holds the labels at
 * the masked positions, as `model(...).output` does.  Snapshot, status, scot_plan_run (pixel_mask NULL) at the current weights and
 * two-stream replay work unchanged on a masked plan.
 * Refused before anything is copied or launched: a format-1/2/5 plan: -3; scot_plan_loss / scot_plan_train_step on a masked plan (the
 * mask is missing), a non-NULL mask on an unmasked training plan, a NULL mask on a masked plan: -1.  On an unmasked training plan with a
 * NULL mask they ARE the unmasked calls. */
int scot_plan_loss_masked(scot_plan_t plan, const float* pixel_values, const float* time, const float* labels, const void* pixel_mask,
                          float* loss, float* prediction, scot_stream_t stream);
int scot_plan_train_step_masked(scot_plan_t plan, const float* pixel_values, const float* time, const float* labels, const void* pixel_mask,
                                const float* lr, float* loss, scot_stream_t stream);

/* ---- gradient accumulation ---- */
/* The arena-wide pass behind the calls below, usable alone.  For every element i with map8[i / 8] != 255 (map8: the optimizer's group
 * map, one byte per 8 floats of the arena, 255 = not a parameter):
 *   acc == NULL: dst[i] = weight * grad[i]            acc != NULL: dst[i] = acc[i] + weight * grad[i]
 * and every other float of dst keeps its bits.  The product is rounded to fp32, then the sum: two roundings, never an FMA — bit for bit
 * what `acc + grad * weight` gives as two eager fp32 torch operations.  With acc == NULL and weight == 1 it is a masked copy that
 * preserves every non-NaN bit pattern (-0.0, denormals, +-Inf).  Inf and NaN go through: a non-finite grad[i] makes exactly dst[i]
 * non-finite.  dst == acc (in place) is allowed; dst must not overlap grad.  One launch on `stream`, 8 floats per lane and 16-byte
 * accesses, no atomics: bitwise repeatable.  -1 (nothing launched, dst untouched): a NULL dst, grad or map8, n == 0 or n % 8 != 0, a
 * dst, acc or grad that is not 16-byte aligned, a non-finite weight, dst == grad; -4: the launch failed. */
int scot_grad_accumulate(float* dst, const float* acc, const float* grad, const unsigned char* map8, size_t n, float weight,
                         scot_stream_t stream);
/* Workgroups that pass launches for n floats (256 lanes each, two 8-float groups per lane and trip: one sweep of the grid covers
 * blocks * 4096 floats, longer arenas take further trips). */
int scot_grad_accumulate_blocks(size_t n);
/* A training step cut between its backward and its update, for an effective batch larger than the recorded one: M micro-batches into
 * an fp32 accumulator A, then ONE update from it.
 *   for k in 0 .. M-1: scot_plan_accumulate(plan, pv_k, t_k, y_k, mask_k, 1.0f / M, k == 0, loss_k, stream);
 *   scot_plan_apply(plan, lr, stream);
 * scot_plan_accumulate is one micro-batch: it copies the batch in exactly as scot_plan_train_step_masked does (same checks and refusals;
 * pixel_mask is NULL exactly on an unmasked plan) and replays the step's forward and backward — the gradient arena then holds this
 * micro-batch's unscaled gradient g, its non-finite values counted as always — then runs scot_grad_accumulate on `stream` (a
 * two-stream plan: after the list has joined): first != 0: A = weight * g, discarding whatever was open; first == 0: A = A + weight * g.
 * loss (device [1], may be NULL) <- the micro-batch's own unweighted loss.  No state buffer changes; the gradient scale does not move
 * during an accumulation.  A: arena_floats of fp32, allocated and zero-filled at the first such call, held until the plan is freed and
 * counted in the described device bytes (-4 if that fails); it is 0 outside the parameter positions.  first == 0 with no accumulation
 * open, or a non-finite weight: -1, nothing launched.
 * scot_plan_apply is the update: it writes lr (HOST memory, as for scot_plan_train_step) into the plan's array, copies A over the
 * gradient arena at the parameter positions (scot_grad_accumulate, weight 1), replays the recorded update unchanged and closes the
 * accumulation.  Clipping, the skip of a non-finite norm, the step counters and the fp16 scale update stay the device's decisions, now
 * made on the accumulated gradient: ONE update, one scale decision, however many micro-batches; scot_plan_train_status reports them as
 * before.  Without an open accumulation, or with a NULL lr: -1, nothing launched.
 * IDENTITY: accumulate(first = 1, weight = 1) followed by apply(lr) is scot_plan_train_step on that batch (x * 1 is exact).
 * INTERACTIONS while an accumulation is open:
 *   scot_plan_run, scot_plan_rollout, scot_plan_loss*, scot_plan_evaluate*   allowed (validation between micro-batches): they write neither A
 *                                                                           nor a state buffer;
 *   scot_plan_train_step*   -1, nothing launched: end the accumulation with scot_plan_apply, or restart it with first != 0;
 *   scot_plan_snapshot      allowed; an open accumulation is not part of an image: after a reload the next call needs first != 0;
 *   scot_plan_poison        also fills A and discards the open accumulation (the next first != 0 call zeroes A again).
 * On a format-1/2/5 plan the calls of this section that take a plan return -3. */
int scot_plan_accumulate(scot_plan_t plan, const float* pixel_values, const float* time, const float* labels, const void* pixel_mask,
                         float weight, int first, float* loss, scot_stream_t stream);
int scot_plan_apply(scot_plan_t plan, const float* lr, scot_stream_t stream);
/* *ptr <- the plan's own device buffer, *floats <- its length, the arena's float count: which == 0 the gradient arena the update reads,
 * which == 1 the accumulator A (-1 while it has never been allocated); any other which: -1.  Valid until the plan is freed.  The host may
 * read and write them in the plan's stream order.  This is the hook for data parallelism: a host with one plan per GPU all-reduces A —
 * with the bucket all-reduce of scot_hip.h, or its own — between the last scot_plan_accumulate and scot_plan_apply, and every rank then
 * takes the same skip decision from the same reduced norm.  Composable, never run on more than one GPU. */
int scot_plan_gradients(scot_plan_t plan, int which, float** ptr, size_t* floats);
/* out[2]: micro-batches in the open accumulation (0: none is open), bytes of the accumulator (0 before it is allocated). */
int scot_plan_accumulation_status(scot_plan_t plan, long long* out);

/* Refused before anything is copied or launched: scot_plan_loss / _train_step / _train_status / _snapshot on a format-1/2 plan: -3
 * (as scot_plan_vjp / scot_plan_rollout_vjp on a training plan); a NULL pixel_values, labels or lr, a NULL loss of scot_plan_loss, a NULL
 * time on a plan with a time input (or a time on one without), a snapshot target that is not this plan's image: -1. */

#ifdef __cplusplus
}
#endif
#endif
