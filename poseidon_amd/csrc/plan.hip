// plan — running a trained model from C: the runtime of exported plans (include/scot_plan.h).
//
// poseidon_amd/plan.py records the engine for one input signature and writes the recording as a relocatable image (plan_image.h: up
// to five lists of C-ABI calls, every device address as (buffer, offset), every stream as a placeholder, the weights and tables by
// value).  This file owns the memory and replays the lists: scot_plan_load validates the image, allocates one slab for all buffers,
// uploads what the image holds by value and builds, for every list the image has, the program of scot_tape_replay (host_tape.hip) with
// the final addresses; a call copies the caller's inputs in, writes the caller's stream into a program's stream slots, replays it
// (`replay`), and copies the results out.  The copies are device-to-device copies and the model's arithmetic is the recorded entry
// points'; the only kernels of this file's own are the two that carry a gradient from one step of scot_plan_rollout_vjp to the next.
//
// FORWARD (every image): scot_plan_run and scot_plan_rollout replay it.
//
// BACKWARD (an ADJOINT plan, image format 2), the recorded frozen-model backward: scot_plan_run replays the differentiable forward,
// which leaves its saved activations in the plan's buffers, and scot_plan_vjp copies a cotangent of the prediction in, writes the
// gradient scale {S, 1/S} into the plan's state buffer on the stream, replays the backward and copies the input gradients out.
// One vjp per run: the backward reuses saved rows.  scot_plan_rollout_vjp is the adjoint of the whole rollout: it keeps no activations
// beyond the caller's predictions (every step's input) and, from the last step to the first, replays the forward to recompute the
// saved rows, forms the step's cotangent, replays the backward and carries the input gradient on.
//
// STEP_FORWARD, STEP_BACKWARD, UPDATE (a TRAINING plan, image format 4), one optimizer step — the forward through the loss, the
// backward with the weight gradients, the optimizer update — with everything a step changes as STATE buffers the image stores by
// value: scot_plan_train_step copies a batch in, writes the caller's learning rates into the host array the recorded scot_adamw_step
// call reads at issue time, and replays the three lists; scot_plan_snapshot reads the state back into the image.  No arithmetic of
// its own: clipping, the skip decision and the fp16 gradient scale are the recorded kernels', on the device.
//
// TWO-STREAM plans (image formats 5 and 6: a format-1 / format-4 image whose lists hold the engine's own two-stream program).  The load
// creates the plan's events (timing disabled; their handles go into the programs once, there) and obtains a side stream: one that is
// MEASURED to run beside the load's stream under the engine's fork / join pattern (scot_stream_overlaps, the C form of
// poseidon_amd/streams.py), or the host's (scot_plan_set_side_stream).  `replay` writes the caller's stream and the side stream into the
// program's stream slots.  Every list of such an image is closed (plan_image.h), so the copies in and out stay on the caller's stream
// and every call above works unchanged.  scot_plan_issue_order is a test aid: it issues a list entry by entry in a given order.
//
// EVALUATION (every image): scot_plan_evaluate is scot_plan_run's forward or scot_plan_rollout's chain with scot_error_sums
// (error_sums.hip) behind every forward: it reads the plan's own output buffer against the caller's targets and leaves per-sample,
// per-channel-group error sums; the predictions need not leave the plan.  Its workspace is allocated at the first such call.
// scot_plan_evaluate_masked takes a pixel_mask of the caller's beside the targets and runs scot_error_sums_masked with overwrite = 1 on
// the output buffer instead: the sums are the masked ones, and the labels under the mask travel on into the next step's input.
//
// PIXEL MASKS (training images): a masked training image (training flag bits 1 and 2) has one more input buffer, the mask bytes the
// recorded scot_head_finalize / scot_loss_bwd entries read; scot_plan_loss_masked / scot_plan_train_step_masked copy the caller's mask
// into it, and the unmasked calls refuse such a plan (the mask is missing).
//
// GRADIENT ACCUMULATION (training images): the step cut between its backward and its update.  scot_plan_accumulate replays the step's
// forward and backward and folds the gradient arena into an fp32 accumulator with scot_grad_accumulate (optim.hip); scot_plan_apply copies
// the accumulator back over the gradient arena with the same kernel and replays the update.  The arena and the group map are arguments
// of the recorded scot_adamw_step entry, resolved at load beside the lr patch point; the accumulator is allocated at the first call.
//
// A plan is one stream's worth of state: its buffers are reused by every run, so runs of ONE plan must be ordered (same stream, or
// the caller's own events); two plans are independent.
#include "common.h"
#include "plan_image.h"
#include <dlfcn.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <string>
#include <vector>

extern "C" int scot_tape_replay(const uint64_t* prog, size_t n_words, int* fail_entry);
extern "C" int scot_abi_version();
extern "C" int scot_operand_format();
extern "C" size_t scot_error_sums_workspace_bytes(int B, int C, int HW, const int* channel_slices, int groups);
extern "C" int scot_error_sums(const float* pred, const float* target, int B, int C, int HW, const int* channel_slices, int groups, double* sums,
                               void* workspace, size_t workspace_bytes, hipStream_t stream);
extern "C" int scot_error_sums_masked(float* pred, const float* target, const unsigned char* mask, int mask_full, int overwrite, int B, int C,
                                      int HW, const int* channel_slices, int groups, double* sums, void* workspace, size_t workspace_bytes,
                                      hipStream_t stream);
extern "C" int scot_grad_accumulate(float* dst, const float* acc, const float* grad, const unsigned char* map8, size_t n, float weight,
                                    hipStream_t stream);

// the listed entry points, by address: g_entry_address[table][index], rows in the order of scot_plan_lists[table].names (the training
// table is the longest: it repeats the forward's)
#define SCOT_PLAN_DECLARE(n) extern "C" int n(...);
SCOT_PLAN_ADJOINT_ENTRY_POINTS(SCOT_PLAN_DECLARE)
SCOT_PLAN_TRAINING_ENTRY_POINTS(SCOT_PLAN_DECLARE)
SCOT_PLAN_SYNC_ENTRY_POINTS(SCOT_PLAN_DECLARE)
#define SCOT_PLAN_ADDRESS(n) (void*)&n,
static void* const g_entry_address[SCOT_PLAN_N_LISTS][SCOT_PLAN_COUNT(scot_plan_training_entry_names)] = {
    {SCOT_PLAN_ENTRY_POINTS(SCOT_PLAN_ADDRESS)}, {SCOT_PLAN_ADJOINT_ENTRY_POINTS(SCOT_PLAN_ADDRESS)}, {SCOT_PLAN_TRAINING_ENTRY_POINTS(SCOT_PLAN_ADDRESS)},
    {SCOT_PLAN_SYNC_ENTRY_POINTS(SCOT_PLAN_ADDRESS)}};

// ------------------------------------------------------------------ device memory and copies (plain host memory in the CPU emulation)
namespace {
enum CopyKind { H2D, D2H, D2D };
#ifdef SCOT_HIPEMU
// the emulated build's launch log: everything the plan runtime has put on a stream — copies, fills and replayed calls — is counted,
// so that a test can see that a refused call issued nothing (scot_plan_emu_issued below; not part of the C ABI)
long long g_emu_issued = 0;
// (as aligned as hipMalloc's memory: kernels choose their vector paths by address, and a plan must take the engine's)
inline void* dev_alloc(size_t n) { return aligned_alloc(256, (n + 255) / 256 * 256); }
inline void dev_free(void* p) { free(p); }
inline bool dev_copy(void* dst, const void* src, size_t n, CopyKind, hipStream_t) { ++g_emu_issued; memmove(dst, src, n); return true; }
inline bool dev_fill(void* dst, int byte, size_t n, hipStream_t) { ++g_emu_issued; memset(dst, byte, n); return true; }
inline bool dev_copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipStream_t) {
  ++g_emu_issued;
  for (size_t r = 0; r < height; ++r) memmove((char*)dst + r * dpitch, (const char*)src + r * spitch, width);
  return true;
}
inline bool dev_sync(hipStream_t) { return true; }
// streams and events of a two-stream plan: stubs (the emulation runs every entry to completion where it is issued)
typedef void* dev_event_t;
inline bool dev_event_create(dev_event_t* e) { *e = (void*)(uintptr_t)1; return true; }
inline void dev_event_destroy(dev_event_t) {}
inline bool dev_stream_create(hipStream_t* s) { *s = (hipStream_t)(uintptr_t)1; return true; }
inline void dev_stream_destroy(hipStream_t) {}
inline int dev_overlaps(hipStream_t, hipStream_t) { return 0; }
// the carry of scot_plan_rollout_vjp as host loops (the kernels further down, element for element)
inline bool dev_carry(float* hold, const float* g, float* hold_t, const float* g_t, size_t B, size_t cin, size_t cout, size_t hw, bool first,
                      bool last, int steps, hipStream_t) {
  ++g_emu_issued;
  if (hold)
    for (size_t i = 0; i < B * cin * hw; ++i) hold[i] = (first || (i / hw) % cin < cout) ? g[i] : hold[i] + g[i];
  if (hold_t)
    for (size_t b = 0; b < B; ++b) {
      const float v = first ? g_t[b] : hold_t[b] + g_t[b];
      hold_t[b] = last ? v / (float)steps : v;      // (torch's CPU kernel divides: scot_plan_rollout)
    }
  return true;
}
inline bool dev_cotangent(float* cot, const float* d_pred, const float* hold, size_t B, size_t cin, size_t cout, size_t hw, hipStream_t) {
  ++g_emu_issued;
  for (size_t b = 0; b < B; ++b)
    for (size_t i = 0; i < cout * hw; ++i) cot[b * cout * hw + i] = d_pred[b * cout * hw + i] + hold[b * cin * hw + i];
  return true;
}
#else
inline void* dev_alloc(size_t n) {
  void* p = nullptr;
  return hipMalloc(&p, n) == hipSuccess ? p : nullptr;
}
inline void dev_free(void* p) { (void)hipFree(p); }
inline bool dev_copy(void* dst, const void* src, size_t n, CopyKind k, hipStream_t s) {
  const hipMemcpyKind kind = k == H2D ? hipMemcpyHostToDevice : (k == D2H ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
  return hipMemcpyAsync(dst, src, n, kind, s) == hipSuccess;
}
inline bool dev_fill(void* dst, int byte, size_t n, hipStream_t s) { return hipMemsetAsync(dst, byte, n, s) == hipSuccess; }
inline bool dev_copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipStream_t s) {
  return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, s) == hipSuccess;
}
inline bool dev_sync(hipStream_t s) { return hipStreamSynchronize(s) == hipSuccess; }
typedef hipEvent_t dev_event_t;
inline bool dev_event_create(dev_event_t* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess; }
inline void dev_event_destroy(dev_event_t e) { (void)hipEventDestroy(e); }
inline bool dev_stream_create(hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess; }
inline void dev_stream_destroy(hipStream_t s) { (void)hipStreamDestroy(s); }

// ---- the stream probe (scot_stream_overlaps).  One wavefront that spins on the constant-rate clock (100 MHz on gfx950) for `ticks`, inside
// a loop bounded by `max_rounds`; it reads nothing and writes nothing.
__global__ __launch_bounds__(64) void plan_spin_kernel(long long ticks, int max_rounds) {
  const long long t0 = (long long)wall_clock64();
  for (int r = 0; r < max_rounds; ++r) {
    if ((long long)wall_clock64() - t0 >= ticks) break;
    __builtin_amdgcn_s_sleep(32);
  }
}
const long long SPIN_TICKS = 50000;      // 0.5 ms: long against event / launch latencies, short against anything a user would notice
const int SPIN_ROUNDS = 1 << 13;         // (a round is at least the sleep's 32 x 64 cycles, ~1 us: the bound is ~20 spins, reached only by a dead clock)
inline void spin(hipStream_t s, long long ticks = SPIN_TICKS) { hipLaunchKernelGGL(plan_spin_kernel, dim3(1), dim3(64), 0, s, ticks, SPIN_ROUNDS); }

// GPU milliseconds on `a` of: K1 on a; b waits for it; K2 on b beside K3 on a; a waits for K2 (`single`: of K1 alone, one kernel time)
inline bool spin_ms(hipStream_t a, hipStream_t b, bool single, hipEvent_t e0, hipEvent_t e1, hipEvent_t fork, hipEvent_t join, float* ms) {
  bool ok = hipEventRecord(e0, a) == hipSuccess;
  spin(a);
  if (!single) {
    ok = ok && hipEventRecord(fork, a) == hipSuccess && hipStreamWaitEvent(b, fork, 0) == hipSuccess;
    spin(b);
    ok = ok && hipEventRecord(join, b) == hipSuccess;
    spin(a);
    ok = ok && hipStreamWaitEvent(a, join, 0) == hipSuccess;
  }
  ok = ok && hipEventRecord(e1, a) == hipSuccess && scot_check_launch() == SCOT_OK;
  ok = ok && hipStreamSynchronize(a) == hipSuccess && (single || hipStreamSynchronize(b) == hipSuccess);
  return ok && hipEventElapsedTime(ms, e0, e1) == hipSuccess;
}

// 1: `b` runs beside `a` under the fork / join pattern — three spin kernels take about two kernel times, the best of two trials; 0: they
// serialise (or a == b); -1: the measurement itself failed
inline int dev_overlaps(hipStream_t a, hipStream_t b) {
  if (a == b) return 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ok = true;
  for (int i = 0; i < 4 && ok; ++i) ok = hipEventCreateWithFlags(&ev[i], i < 2 ? hipEventDefault : hipEventDisableTiming) == hipSuccess;
  // (both streams are used once first: the runtime attaches a stream to its hardware queue at its first submission)
  if (ok) {
    spin(a, 100);
    spin(b, 100);
    ok = hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess;
  }
  float one = 0.0f, best = 0.0f, ms = 0.0f;
  ok = ok && spin_ms(a, b, true, ev[0], ev[1], ev[2], ev[3], &one);
  for (int trial = 0; trial < 2 && ok; ++trial) {
    ok = spin_ms(a, b, false, ev[0], ev[1], ev[2], ev[3], &ms);
    best = trial == 0 || ms < best ? ms : best;
  }
  for (int i = 0; i < 4; ++i)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  return ok ? (best < 2.5f * one ? 1 : 0) : -1;
}

// ---- the carry of scot_plan_rollout_vjp: the only kernels the plan runtime launches itself.  Internal (no entry points of scot_hip.h);
// T = float4 where every (sample, channel) plane is a whole number of 16-byte aligned vectors, float otherwise.  Plain fp32 adds in the
// order scot_plan.h fixes; plain vector stores.
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vadd(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// after one backward: hold [B, Cin, plane] <- the step's input gradient g — moved on the first Cout channels (the next cotangent's
// carry), accumulated on the pass-through channels (hold + g; moved by the first backward of the sweep); hold_t [B] <- hold_t + g_t
// (moved by the first backward), times 1 / steps in the last one.  hold / hold_t may be NULL.  n, plane in units of T.
template <typename T>
__global__ __launch_bounds__(256) void plan_carry_kernel(T* __restrict__ hold, const T* __restrict__ g, float* __restrict__ hold_t,
                                                         const float* __restrict__ g_t, size_t n, size_t plane, unsigned cin, unsigned cout,
                                                         unsigned B, int first, int last, float inv_steps) {
  const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  if (hold_t)
    for (size_t b = t0; b < B; b += stride) {
      const float v = first ? g_t[b] : hold_t[b] + g_t[b];
      hold_t[b] = last ? v * inv_steps : v;      // (torch's GPU kernel multiplies by the reciprocal: scot_plan_rollout)
    }
  if (hold)
    for (size_t i = t0; i < n; i += stride) {
      const T v = g[i];
      hold[i] = (first || (i / plane) % cin < cout) ? v : vadd(hold[i], v);
    }
}
// after the next forward: cot [B, Cout, plane] <- d_pred [B, Cout, plane] + hold[:, :Cout] (hold's sample pitch is Cin planes)
template <typename T>
__global__ __launch_bounds__(256) void plan_cotangent_kernel(T* __restrict__ cot, const T* __restrict__ d_pred, const T* __restrict__ hold,
                                                             size_t n, size_t out_row, size_t in_row) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / out_row;
    cot[i] = vadd(d_pred[i], hold[b * in_row + (i - b * out_row)]);
  }
}
inline unsigned carry_blocks(size_t n) {
  const size_t blocks = (n + 255) / 256;
  return (unsigned)(blocks > 4096 ? 4096 : (blocks ? blocks : 1));
}
inline bool vec4_ok(size_t hw, const void* a, const void* b, const void* c) {
  return hw % 4 == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0);
}
inline bool dev_carry(float* hold, const float* g, float* hold_t, const float* g_t, size_t B, size_t cin, size_t cout, size_t hw, bool first,
                      bool last, int steps, hipStream_t s) {
  const float inv_steps = 1.0f / (float)steps;
  const size_t n = hold ? B * cin * hw : B;
  if (vec4_ok(hw, hold, g, nullptr))
    hipLaunchKernelGGL(plan_carry_kernel<float4>, dim3(carry_blocks(n / 4)), dim3(256), 0, s, (float4*)hold, (const float4*)g, hold_t, g_t, n / 4,
                       hw / 4, (unsigned)cin, (unsigned)cout, (unsigned)B, (int)first, (int)last, inv_steps);
  else
    hipLaunchKernelGGL(plan_carry_kernel<float>, dim3(carry_blocks(n)), dim3(256), 0, s, hold, g, hold_t, g_t, n, hw, (unsigned)cin,
                       (unsigned)cout, (unsigned)B, (int)first, (int)last, inv_steps);
  return scot_check_launch() == SCOT_OK;
}
inline bool dev_cotangent(float* cot, const float* d_pred, const float* hold, size_t B, size_t cin, size_t cout, size_t hw, hipStream_t s) {
  const size_t n = B * cout * hw;
  if (vec4_ok(hw, cot, d_pred, hold))
    hipLaunchKernelGGL(plan_cotangent_kernel<float4>, dim3(carry_blocks(n / 4)), dim3(256), 0, s, (float4*)cot, (const float4*)d_pred,
                       (const float4*)hold, n / 4, cout * hw / 4, cin * hw / 4);
  else
    hipLaunchKernelGGL(plan_cotangent_kernel<float>, dim3(carry_blocks(n)), dim3(256), 0, s, cot, d_pred, hold, n, cout * hw, cin * hw);
  return scot_check_launch() == SCOT_OK;
}
#endif

const uint64_t PLAN_HANDLE_MAGIC = 0x50414c5053434f54ull;
// scot_adamw_step(params, GRADS, exp_avg, exp_avg_sq, MAP8, n, lr, ...): what the accumulation calls take from the recorded entry
const uint64_t SCOT_PLAN_ADAMW_GRAD_ARG = 1, SCOT_PLAN_ADAMW_MAP_ARG = 4;
const size_t SLAB_ALIGN = 256, SLAB_TAIL = 64 << 10;

struct Plan {
  uint64_t magic = PLAN_HANDLE_MAGIC;
  char* slab = nullptr;
  size_t slab_bytes = 0;
  std::vector<char*> buf;                          // start of every buffer inside the slab
  std::vector<uint64_t> buf_kind, buf_bytes;
  struct Program {
    std::vector<uint64_t> prog;                    // scot_tape_replay's word format, final addresses
    std::vector<size_t> stream_slot;               // words of prog that hold a stream ...
    std::vector<uint8_t> slot_stream;              // ... and which: 0 = the caller's, 1 = the plan's side stream
    std::vector<size_t> entry_at;                  // two-stream plans: the word offset of every entry in prog (and prog's end) ...
    std::vector<uint8_t> entry_stream;             // ... and the stream it is issued on
    std::vector<int> order;                        // scot_plan_issue_order: the order later replays issue the entries in (empty: as recorded)
    uint64_t calls = 0;
  } list[SCOT_PLAN_N_CALLS];                       // SCOT_PLAN_CALLS_*; a list the image does not have is empty
  // two-stream plans (formats 5 and 6): the events and the side stream, whether the load created it, whether it was measured to run beside
  // the load's stream, and whether a list has been issued (the side stream is fixed from then on)
  uint64_t n_streams = 1;
  std::vector<dev_event_t> events;
  hipStream_t side = nullptr, load_stream = nullptr;
  bool side_own = false, side_host = false, started = false;
  int side_overlaps = 0;
  std::vector<std::vector<uint64_t>> host_arrays;  // host arrays the entries pass by address: pointers, or packed int32 / float
  // training plans: the training words, where the update reads lr[groups], and what scot_plan_snapshot compares a target image with
  // and writes into (the header, the buffer table, each stored buffer's place)
  uint64_t train[SCOT_PLAN_TRAIN_WORDS] = {};
  float* lr = nullptr;
  uint64_t header[SCOT_PLAN_HEADER_WORDS] = {};
  std::vector<uint64_t> buffer_table;
  std::vector<float> host_time;                    // scot_plan_rollout: the divided time on its way back to the device
  uint64_t io[SCOT_PLAN_IO_WORDS] = {};
  uint64_t adj[SCOT_PLAN_ADJ_WORDS] = {};
  int operand_format = 0, compute = 0, format = SCOT_PLAN_FORMAT;      // format: the ONE-stream format (1, 2, 4) the image extends
  long long resize[4] = {0, 0, 0, 0};              // scot_plan_describe_resize: read from the forward list at load (read_resize)
  bool ran = false;                                // a completed scot_plan_run whose saved activations no vjp / poison / rollout has used up
  float host_scale[4] = {1.0f, 1.0f, 0.0f, 0.0f};  // {S, 1/S, 0, 0} on its way to the state buffer
  int last_exponent = 0;                           // log2 S of the last vjp
  float* holder = nullptr;                         // scot_plan_rollout_vjp without a d_pixel_values of the caller's: the carry's [B, Cin, H, W]
  size_t holder_bytes = 0;
  void* eval_ws = nullptr;                         // scot_plan_evaluate: the workspace of scot_error_sums, for any slices over Cout channels
  size_t eval_ws_bytes = 0;
  // gradient accumulation: what the recorded scot_adamw_step reads as its gradients and its group map (resolved at load; NULL where the
  // entry does not hold them as spans of the plan's buffers), the fp32 accumulator A of arena_floats (allocated at the first
  // scot_plan_accumulate), the micro-batches of the open accumulation (0: none is open), and whether scot_plan_poison has filled A
  float* grad_arena = nullptr;
  const unsigned char* group_map = nullptr;
  float* accum = nullptr;
  size_t accum_bytes = 0;
  long long accum_open = 0;
  bool accum_poisoned = false;
};

inline Plan* as_plan(void* p) {
  Plan* pl = (Plan*)p;
  return pl && pl->magic == PLAN_HANDLE_MAGIC ? pl : nullptr;
}

// The bfloat16 build of this library, for entries recorded there (plan_image.h: library 1).  The bfloat16 build is its own peer.
void* g_peer = nullptr;

void* open_peer(const char* path) {
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) return nullptr;
  typedef int (*query_t)();
  query_t fmt = (query_t)dlsym(h, "scot_operand_format"), abi = (query_t)dlsym(h, "scot_abi_version");
  if (!fmt || !abi || fmt() != 0 || abi() != scot_abi_version()) {
    dlclose(h);
    return nullptr;
  }
  return h;
}

// the library next to this one (libscot_hip.so beside libscot_hip_f16.so), unless scot_plan_peer_library named another
void* default_peer() {
  Dl_info info;
  if (!dladdr((void*)&scot_operand_format, &info) || !info.dli_fname) return nullptr;
  std::string dir(info.dli_fname);
  const size_t slash = dir.rfind('/');
  dir = slash == std::string::npos ? std::string(".") : dir.substr(0, slash);
  return open_peer((dir + "/libscot_hip.so").c_str());
}

void* resolve(const char* name, uint64_t lib, int list, bool streamed) {
  int index = scot_plan_list_index(name, list);
  if (index < 0 && streamed && (index = scot_plan_list_index(name, SCOT_PLAN_LIST_SYNC)) >= 0) list = SCOT_PLAN_LIST_SYNC;
  if (index < 0) return nullptr;
  if (lib == 0 || scot_operand_format() == 0) return g_entry_address[list][index];
  if (!g_peer) g_peer = default_peer();
  return g_peer ? dlsym(g_peer, name) : nullptr;
}

// one argument pair -> the word the call receives; a stream is a placeholder (patched per run), an event is the plan's own
bool materialise(Plan* pl, uint64_t tagw, uint64_t val, uint64_t* out, bool* is_stream) {
  *is_stream = false;
  switch (tagw & 0xff) {
    case SCOT_PLAN_ARG_INT: *out = val; return true;
    case SCOT_PLAN_ARG_NULL: *out = 0; return true;
    case SCOT_PLAN_ARG_PTR: *out = (uint64_t)(uintptr_t)(pl->buf[tagw >> 8] + val); return true;
    case SCOT_PLAN_ARG_STREAM: *out = 0; *is_stream = true; return true;
    case SCOT_PLAN_ARG_EVENT: *out = (uint64_t)(uintptr_t)pl->events[val]; return true;
    default: return false;
  }
}

// one of the plan's lists (SCOT_PLAN_CALLS_*) on `stream` (and, a two-stream plan, its side stream): as recorded in one run of
// scot_tape_replay, or — scot_plan_issue_order — entry by entry in the installed order, both streams synchronised at every switch
int replay(Plan* pl, int list, hipStream_t stream) {
  Plan::Program& p = pl->list[list];
  const hipStream_t streams[2] = {stream, pl->side};
  for (size_t k = 0; k < p.stream_slot.size(); ++k) p.prog[p.stream_slot[k]] = (uint64_t)(uintptr_t)streams[p.slot_stream[k]];
  pl->started = true;
#ifdef SCOT_HIPEMU
  g_emu_issued += (long long)p.calls;
#endif
  int fail = -1;
  if (p.order.empty()) return scot_tape_replay(p.prog.data(), p.prog.size(), &fail);
  int prev = -1;
  for (int j : p.order) {
    const int on = p.entry_stream[j];
    if (prev >= 0 && on != prev && !(dev_sync(stream) && dev_sync(pl->side))) return SCOT_ERR_LAUNCH;
    const int rc = scot_tape_replay(p.prog.data() + p.entry_at[j], p.entry_at[j + 1] - p.entry_at[j], &fail);
    if (rc != SCOT_OK) return rc;
    prev = on;
  }
  return dev_sync(stream) && dev_sync(pl->side) ? SCOT_OK : SCOT_ERR_LAUNCH;
}

// one call list -> the entry points' addresses (false: one is missing)
bool resolve_section(const scot_plan_view& v, const scot_plan_calls& c, std::vector<void*>* fn) {
  fn->resize(c.n);
  const uint64_t* e = c.words;
  for (uint64_t i = 0; i < c.n; ++i, e += scot_plan_entry_words(e)) {
    (*fn)[i] = resolve((const char*)(v.names + e[0] * SCOT_PLAN_NAME_BYTES), e[1], c.names, v.n_streams > 1);
    if (!(*fn)[i]) return false;
  }
  return true;
}

// one call list -> scot_tape_replay's program with the final addresses
bool build_program(Plan* pl, const scot_plan_calls& c, const std::vector<void*>& fn, const std::vector<uint64_t>& array_address,
                   Plan::Program* out) {
  out->calls = c.n;
  out->prog.reserve((size_t)(c.n_words + c.n));
  const uint64_t* e = c.words;
  for (uint64_t i = 0; i < c.n; ++i, e += scot_plan_entry_words(e)) {
    const uint64_t ni = e[2], nf = e[3];
    out->entry_at.push_back(out->prog.size());
    out->entry_stream.push_back(0);
    out->prog.push_back((uint64_t)(uintptr_t)fn[i]);
    out->prog.push_back(ni);
    out->prog.push_back(nf);
    for (uint64_t k = 0; k < ni; ++k) {
      const uint64_t tagw = e[4 + 2 * k], val = e[5 + 2 * k];
      uint64_t word = 0;
      bool st = false;
      if ((tagw & 0xff) == SCOT_PLAN_ARG_ARRAY)
        word = array_address[val];
      else if (!materialise(pl, tagw, val, &word, &st))
        return false;
      if (st) {
        out->stream_slot.push_back(out->prog.size());
        out->slot_stream.push_back((uint8_t)val);
        out->entry_stream.back() = (uint8_t)val;
      }
      out->prog.push_back(word);
    }
    for (uint64_t k = 0; k < nf; ++k) out->prog.push_back(e[4 + 2 * ni + k]);
  }
  out->entry_at.push_back(out->prog.size());
  return true;
}

// A plan at a foreign resolution (export_plan(..., resize=True)) has no header word of its own: its forward list starts with a
// scot_spectral_resize(X, Pr, Pi, Y, nimg, s, t, stream) entry from the host's resolution s to the model's t.  -> {resized, native size,
// host size, resize entries in all lists}; an image without such a first entry runs at its native size H.
void read_resize(const scot_plan_view& v, long long out[4]) {
  const long long H = (long long)v.io[SCOT_PLAN_IO_H];
  out[0] = 0; out[1] = H; out[2] = H; out[3] = 0;
  for (int c = 0; c < SCOT_PLAN_N_CALLS; ++c) {
    const uint64_t* e = v.calls[c].words;
    for (uint64_t i = 0; i < v.calls[c].n; ++i, e += scot_plan_entry_words(e)) {
      if (strcmp((const char*)(v.names + e[0] * SCOT_PLAN_NAME_BYTES), "scot_spectral_resize") != 0) continue;
      ++out[3];
      if (c == SCOT_PLAN_CALLS_FORWARD && i == 0 && e[2] >= 7 && (e[4 + 2 * 6] & 0xff) == SCOT_PLAN_ARG_INT) {
        out[0] = 1;
        out[1] = (long long)e[5 + 2 * 6];      // t of the first entry: what the engine runs at
      }
    }
  }
}

// the address of a (buffer, offset, bytes) span of the adjoint or training words (pl->adj, pl->train)
char* span_ptr(Plan* pl, const uint64_t* words, int slot) { return pl->buf[words[slot]] + words[slot + 1]; }

// ... and of a (buffer, offset) pair of the io words
char* io_ptr(Plan* pl, int buf_word) { return span_ptr(pl, pl->io, buf_word); }

const char* listed_name(int list, int i) { return i >= 0 && i < scot_plan_lists[list].count ? scot_plan_lists[list].names[i] : nullptr; }
}  // namespace

extern "C" const char* scot_plan_entry_point(int i) { return listed_name(SCOT_PLAN_LIST_FORWARD, i); }
extern "C" const char* scot_plan_adjoint_entry_point(int i) { return listed_name(SCOT_PLAN_LIST_ADJOINT, i); }
extern "C" const char* scot_plan_training_entry_point(int i) { return listed_name(SCOT_PLAN_LIST_TRAINING, i); }
#ifdef SCOT_HIPEMU
extern "C" long long scot_plan_emu_issued() { return g_emu_issued; }
#endif

extern "C" int scot_plan_peer_library(const char* path) {
  if (!path) return SCOT_ERR_SHAPE;
  void* h = open_peer(path);
  if (!h) return SCOT_ERR_UNSUPPORTED;
  g_peer = h;      // (a previous handle stays open: plans loaded through it hold its addresses)
  return SCOT_OK;
}

extern "C" int scot_plan_free(void* plan) {
  Plan* pl = as_plan(plan);
  if (!pl) return plan ? SCOT_ERR_SHAPE : SCOT_OK;
  if (pl->slab) dev_free(pl->slab);
  if (pl->holder) dev_free(pl->holder);
  if (pl->eval_ws) dev_free(pl->eval_ws);
  if (pl->accum) dev_free(pl->accum);
  for (dev_event_t e : pl->events) dev_event_destroy(e);
  if (pl->side_own) dev_stream_destroy(pl->side);
  pl->magic = 0;
  delete pl;
  return SCOT_OK;
}

extern "C" int scot_plan_load(const void* image, size_t bytes, void** plan, hipStream_t stream) {
  if (!plan) return SCOT_ERR_SHAPE;
  *plan = nullptr;
#if !defined(__x86_64__) || defined(_WIN32)
  (void)image; (void)bytes; (void)stream;
  return SCOT_ERR_UNSUPPORTED;      // where scot_tape_replay is (host_tape.hip)
#else
  scot_plan_view v;
  const int rc = scot_plan_image_validate(image, bytes, scot_abi_version(), scot_operand_format(), &v);
  if (rc != SCOT_PLAN_OK) return rc;
  Plan* pl = new (std::nothrow) Plan;
  if (!pl) return SCOT_ERR_LAUNCH;
  int status = SCOT_OK;
  try {
    memcpy(pl->io, v.io, sizeof(pl->io));
    read_resize(v, pl->resize);
    pl->format = v.format == SCOT_PLAN_FORMAT_STREAMS ? SCOT_PLAN_FORMAT : (v.format == SCOT_PLAN_FORMAT_TRAINING_STREAMS ? SCOT_PLAN_FORMAT_TRAINING : (int)v.format);
    pl->n_streams = v.n_streams;
    pl->load_stream = stream;
    if (v.adj) memcpy(pl->adj, v.adj, sizeof(pl->adj));
    if (v.train) memcpy(pl->train, v.train, sizeof(pl->train));
    memcpy(pl->header, v.h, sizeof(pl->header));
    pl->buffer_table.assign(v.buffers, v.buffers + 4 * v.n_buffers);
    pl->operand_format = (int)v.h[SCOT_PLAN_H_OPERAND];
    pl->compute = (int)v.h[SCOT_PLAN_H_COMPUTE];
    // every entry point, before anything is allocated
    std::vector<void*> fn[SCOT_PLAN_N_CALLS];
    for (int c = 0; c < SCOT_PLAN_N_CALLS; ++c)
      if (!resolve_section(v, v.calls[c], &fn[c])) status = SCOT_ERR_UNSUPPORTED;
    // one slab, every buffer on a 256-byte boundary
    std::vector<size_t> off(v.n_buffers);
    size_t total = 0;
    for (uint64_t i = 0; i < v.n_buffers; ++i) {
      off[i] = total;
      total += (size_t)((v.buffers[4 * i + 1] + SLAB_ALIGN - 1) / SLAB_ALIGN * SLAB_ALIGN);
    }
    if (status == SCOT_OK) {
      // (one tile of room behind the last buffer: a kernel's vector load may run a few elements past the rows it was given, as it may
      // inside a caching allocator's block)
      pl->slab = (char*)dev_alloc(total + SLAB_TAIL);
      pl->slab_bytes = total;
      if (!pl->slab) status = SCOT_ERR_LAUNCH;
    }
    if (status == SCOT_OK) {
      for (uint64_t i = 0; i < v.n_buffers; ++i) {
        pl->buf.push_back(pl->slab + off[i]);
        pl->buf_kind.push_back(v.buffers[4 * i]);
        pl->buf_bytes.push_back(v.buffers[4 * i + 1]);
      }
      // (scratch is zeroed once so that a first run never reads bytes of whoever held the memory before; scot_plan_poison overwrites it)
      if (!dev_fill(pl->slab, 0, total, stream)) status = SCOT_ERR_LAUNCH;
      for (uint64_t i = 0; i < v.n_buffers && status == SCOT_OK; ++i)
        if ((v.buffers[4 * i] == SCOT_PLAN_BUF_CONSTANT || (v.buffers[4 * i] == SCOT_PLAN_BUF_STATE && v.train && v.buffers[4 * i + 3] == 1)) &&
            !dev_copy(pl->buf[i], v.data + v.buffers[4 * i + 2], (size_t)v.buffers[4 * i + 1], H2D, stream))
          status = SCOT_ERR_LAUNCH;
    }
    // host arrays, with their final contents: pointers (kind 1) as words, int32 (0) and float bits (2) packed, four bytes each
    std::vector<uint64_t> array_address;
    if (status == SCOT_OK) {
      uint64_t w = 0;
      for (uint64_t i = 0; i < v.n_arrays; ++i) {
        const uint64_t kind = v.arrays[w], cnt = v.arrays[w + 1];
        std::vector<uint64_t> a((size_t)(kind == 1 ? cnt : (cnt + 1) / 2) + 1);
        for (uint64_t k = 0; k < cnt; ++k) {
          const uint64_t tagw = v.arrays[w + 2 + 2 * k], val = v.arrays[w + 3 + 2 * k];
          const uint32_t low = (uint32_t)val;
          bool st;
          if (kind != 1)
            memcpy((char*)a.data() + 4 * k, &low, 4);
          else if (!materialise(pl, tagw, val, &a[k], &st))
            status = SCOT_ERR_SHAPE;
        }
        pl->host_arrays.push_back(std::move(a));
        array_address.push_back((uint64_t)(uintptr_t)pl->host_arrays.back().data());
        w += 2 + 2 * cnt;
      }
    }
    // a two-stream plan's events, and a side stream that runs beside `stream`: the first of up to eight candidates that is measured to
    // (scot_stream_overlaps); if none is, the first candidate — the plan is then correct but may serialise, and says so
    // (scot_plan_describe_streams).  Never a reason to fail the load.
    if (status == SCOT_OK && v.n_streams > 1) {
      for (uint64_t i = 0; i < v.n_events && status == SCOT_OK; ++i) {
        dev_event_t e;
        if (dev_event_create(&e)) pl->events.push_back(e);
        else status = SCOT_ERR_LAUNCH;
      }
      std::vector<hipStream_t> tried;
      for (int t = 0; t < 8 && status == SCOT_OK && !pl->side_overlaps; ++t) {
        hipStream_t s;
        if (!dev_stream_create(&s)) {
          if (tried.empty()) status = SCOT_ERR_LAUNCH;
          break;
        }
        tried.push_back(s);
        pl->side_overlaps = dev_overlaps(stream, s) == 1;
      }
      if (!tried.empty()) {
        pl->side = pl->side_overlaps ? tried.back() : tried.front();
        pl->side_own = true;
        for (hipStream_t s : tried)
          if (s != pl->side) dev_stream_destroy(s);
      }
    }
    // the programs
    for (int c = 0; c < SCOT_PLAN_N_CALLS && status == SCOT_OK; ++c)
      if (!build_program(pl, v.calls[c], fn[c], array_address, &pl->list[c])) status = SCOT_ERR_SHAPE;
    if (status == SCOT_OK && v.train) {      // where the recorded scot_adamw_step reads lr[groups] (validated: an array of that many floats)
      const uint64_t* upd = v.calls[SCOT_PLAN_CALLS_UPDATE].words;
      const uint64_t* e = upd + scot_plan_entry_at(upd, v.train[SCOT_PLAN_TR_LR_ENTRY]);
      pl->lr = (float*)(uintptr_t)array_address[e[5 + 2 * v.train[SCOT_PLAN_TR_LR_ARG]]];
      // the same entry's gradients (argument 1) and group map (argument 4), for scot_plan_accumulate / _apply: spans of the plan's own
      // buffers that hold the whole arena, or the accumulation calls refuse
      const uint64_t floats = v.train[SCOT_PLAN_TR_ARENA_FLOATS];
      const uint64_t gt = e[4 + 2 * SCOT_PLAN_ADAMW_GRAD_ARG], go = e[5 + 2 * SCOT_PLAN_ADAMW_GRAD_ARG];
      const uint64_t mt = e[4 + 2 * SCOT_PLAN_ADAMW_MAP_ARG], mo = e[5 + 2 * SCOT_PLAN_ADAMW_MAP_ARG];
      if (e[2] > SCOT_PLAN_ADAMW_MAP_ARG && (gt & 0xff) == SCOT_PLAN_ARG_PTR && (mt & 0xff) == SCOT_PLAN_ARG_PTR && floats && floats % 8 == 0 &&
          go % 16 == 0 && go + floats * 4 <= pl->buf_bytes[gt >> 8] && mo + floats / 8 <= pl->buf_bytes[mt >> 8]) {
        pl->grad_arena = (float*)(pl->buf[gt >> 8] + go);
        pl->group_map = (const unsigned char*)(pl->buf[mt >> 8] + mo);
      }
    }
    // the image may be released when this returns: the uploads read it
    if (status == SCOT_OK && !dev_sync(stream)) status = SCOT_ERR_LAUNCH;
  } catch (const std::bad_alloc&) {
    status = SCOT_ERR_LAUNCH;
  }
  if (status != SCOT_OK) {
    if (pl->slab) (void)dev_sync(stream);
    scot_plan_free(pl);
    return status;
  }
  *plan = pl;
  return SCOT_OK;
#endif
}

// out[16]: batch, input channels, H, W, output channels, time is an input, its bytes, pixel_mask is an input, its bytes, operand format,
// compute mode, bytes of device memory held, recorded calls, bytes of pixel_values, bytes of the prediction, image format version
extern "C" int scot_plan_describe(void* plan, long long* out) {
  Plan* pl = as_plan(plan);
  if (!pl || !out) return SCOT_ERR_SHAPE;
  const uint64_t* io = pl->io;
  const uint64_t hw = io[SCOT_PLAN_IO_H] * io[SCOT_PLAN_IO_W] * io[SCOT_PLAN_IO_B] * 4;
  const long long d[16] = {(long long)io[SCOT_PLAN_IO_B], (long long)io[SCOT_PLAN_IO_CIN], (long long)io[SCOT_PLAN_IO_H],
                           (long long)io[SCOT_PLAN_IO_W], (long long)io[SCOT_PLAN_IO_COUT], (long long)io[SCOT_PLAN_IO_HAS_TIME],
                           (long long)(io[SCOT_PLAN_IO_HAS_TIME] ? io[SCOT_PLAN_IO_TIME_BYTES] : 0), (long long)io[SCOT_PLAN_IO_HAS_MASK],
                           (long long)(io[SCOT_PLAN_IO_HAS_MASK] ? io[SCOT_PLAN_IO_MASK_BYTES] : 0), pl->operand_format, pl->compute,
                           (long long)(pl->slab_bytes + pl->holder_bytes + pl->eval_ws_bytes + pl->accum_bytes), (long long)pl->list[SCOT_PLAN_CALLS_FORWARD].calls, (long long)(hw * io[SCOT_PLAN_IO_CIN]),
                           (long long)(hw * io[SCOT_PLAN_IO_COUT]), (long long)pl->header[SCOT_PLAN_H_FORMAT]};
  memcpy(out, d, sizeof(d));
  return SCOT_OK;
}

// out[4]: the plan resamples its input and its prediction (0 / 1), the size the model runs at, the size the host's tensors have (H = W of
// scot_plan_describe), scot_spectral_resize entries in all call lists
extern "C" int scot_plan_describe_resize(void* plan, long long* out) {
  Plan* pl = as_plan(plan);
  if (!pl || !out) return SCOT_ERR_SHAPE;
  memcpy(out, pl->resize, sizeof(pl->resize));
  return SCOT_OK;
}

// every scratch buffer, the prediction's buffer and the gradient accumulator <- byte (a test aid: with 0xff a run that reads what it did not write yields NaN)
extern "C" int scot_plan_poison(void* plan, int byte, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  pl->ran = false;      // (the saved activations are scratch)
  for (size_t i = 0; i < pl->buf.size(); ++i)
    if (pl->buf_kind[i] == SCOT_PLAN_BUF_SCRATCH || pl->buf_kind[i] == SCOT_PLAN_BUF_OUTPUT)
      if (!dev_fill(pl->buf[i], byte, (size_t)((pl->buf_bytes[i] + SLAB_ALIGN - 1) / SLAB_ALIGN * SLAB_ALIGN), stream)) return SCOT_ERR_LAUNCH;
  pl->accum_open = 0;      // (an open accumulation is discarded, and the accumulator filled: the next first micro-batch zeroes it again)
  if (pl->accum) {
    pl->accum_poisoned = true;
    if (!dev_fill(pl->accum, byte, pl->accum_bytes, stream)) return SCOT_ERR_LAUNCH;
  }
  return SCOT_OK;
}

// the caller's input pointers: pixel_values and `other` (where the result goes, or a batch's labels) are required; time, and with
// `masked` pixel_mask, have to be given exactly where the plan takes them.  (The mask input of a masked TRAINING plan belongs to its step
// lists: the inference list does not read it, so scot_plan_run / scot_plan_rollout on such a plan take NULL as well.)
static int check_inputs(Plan* pl, const void* pixel_values, const void* time, const void* pixel_mask, const void* other, bool masked = true) {
  if (!pixel_values || !other) return SCOT_ERR_SHAPE;
  if ((pl->io[SCOT_PLAN_IO_HAS_TIME] != 0) != (time != nullptr)) return SCOT_ERR_SHAPE;
  const bool optional = pl->format == SCOT_PLAN_FORMAT_TRAINING && !pixel_mask;
  if (masked && !optional && (pl->io[SCOT_PLAN_IO_HAS_MASK] != 0) != (pixel_mask != nullptr)) return SCOT_ERR_SHAPE;
  return SCOT_OK;
}

// the inputs -> the plan's input copies (the caller has checked the pointers; a NULL time or pixel_mask is not copied)
static bool copy_inputs(Plan* pl, const void* pixel_values, const void* time, const void* pixel_mask, hipStream_t stream) {
  const uint64_t* io = pl->io;
  const size_t in_bytes = (size_t)(io[SCOT_PLAN_IO_B] * io[SCOT_PLAN_IO_CIN] * io[SCOT_PLAN_IO_H] * io[SCOT_PLAN_IO_W] * 4);
  if (!dev_copy(io_ptr(pl, SCOT_PLAN_IO_PV_BUF), pixel_values, in_bytes, D2D, stream)) return false;
  if (time && !dev_copy(io_ptr(pl, SCOT_PLAN_IO_TIME_BUF), time, (size_t)io[SCOT_PLAN_IO_TIME_BYTES], D2D, stream)) return false;
  return !pixel_mask || dev_copy(io_ptr(pl, SCOT_PLAN_IO_MASK_BUF), pixel_mask, (size_t)io[SCOT_PLAN_IO_MASK_BYTES], D2D, stream);
}

extern "C" int scot_plan_run(void* plan, const float* pixel_values, const float* time, const void* pixel_mask, float* prediction,
                             hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  int rc = check_inputs(pl, pixel_values, time, pixel_mask, prediction);
  if (rc != SCOT_OK) return rc;
  pl->ran = false;
  const uint64_t* io = pl->io;
  const size_t out_bytes = (size_t)(io[SCOT_PLAN_IO_B] * io[SCOT_PLAN_IO_COUT] * io[SCOT_PLAN_IO_H] * io[SCOT_PLAN_IO_W] * 4);
  if (!copy_inputs(pl, pixel_values, time, pixel_mask, stream)) return SCOT_ERR_LAUNCH;
  rc = replay(pl, SCOT_PLAN_CALLS_FORWARD, stream);
  if (rc != SCOT_OK) return rc;
  if (!dev_copy(prediction, io_ptr(pl, SCOT_PLAN_IO_OUT_BUF), out_bytes, D2D, stream)) return SCOT_ERR_LAUNCH;
  pl->ran = pl->list[SCOT_PLAN_CALLS_BACKWARD].calls != 0;
  return SCOT_OK;
}

// out[8]: has adjoint, d_pixel_values available, d_time available, recorded backward calls, bytes kept between run and vjp, default
// gradient scale (export-time value, as an integer power-of-two exponent), 0, 0.  Format-1 plan: all zeros, status 0.
extern "C" int scot_plan_describe_adjoint(void* plan, long long* out) {
  Plan* pl = as_plan(plan);
  if (!pl || !out) return SCOT_ERR_SHAPE;
  memset(out, 0, 8 * sizeof(long long));
  if (pl->format != SCOT_PLAN_FORMAT_ADJOINT) return SCOT_OK;
  out[0] = 1;
  out[1] = (long long)(pl->adj[SCOT_PLAN_ADJ_FLAGS] & 1);
  out[2] = (long long)((pl->adj[SCOT_PLAN_ADJ_FLAGS] >> 1) & 1);
  out[3] = (long long)pl->list[SCOT_PLAN_CALLS_BACKWARD].calls;
  out[4] = (long long)pl->adj[SCOT_PLAN_ADJ_KEPT_BYTES];
  out[5] = (long long)(int64_t)pl->adj[SCOT_PLAN_ADJ_SCALE_EXP];
  return SCOT_OK;
}

// grad_scale of a vjp -> log2 S: 0 = the export-time value, otherwise a power of two whose reciprocal is a normal float too, and 1 on a
// plan whose backward runs unscaled (fp32 / bf16 / bf16x3).  false: refused.
static bool scale_exponent(const Plan* pl, float grad_scale, int* exponent) {
  *exponent = (int)(int64_t)pl->adj[SCOT_PLAN_ADJ_SCALE_EXP];
  if (grad_scale == 0.0f) return true;
  int e = 0;
  if (!(grad_scale > 0.0f) || !__builtin_isfinite(grad_scale) || frexpf(grad_scale, &e) != 0.5f) return false;
  if (!pl->adj[SCOT_PLAN_ADJ_STATE + 2] && grad_scale != 1.0f) return false;
  if (e - 1 < -120 || e - 1 > 120) return false;
  *exponent = e - 1;
  return true;
}

// {S, 1/S, 0, 0} -> the plan's scale state on `stream` (plans whose backward runs under a scale)
static bool write_scale(Plan* pl, int exponent, hipStream_t stream) {
  pl->last_exponent = exponent;
  if (!pl->adj[SCOT_PLAN_ADJ_STATE + 2]) return true;
  pl->host_scale[0] = ldexpf(1.0f, exponent);
  pl->host_scale[1] = ldexpf(1.0f, -exponent);
  pl->host_scale[2] = pl->host_scale[3] = 0.0f;
  // (host_scale is pageable memory: the runtime has staged it by the time the copy call returned)
  return dev_copy(span_ptr(pl, pl->adj, SCOT_PLAN_ADJ_STATE), pl->host_scale, sizeof(pl->host_scale), H2D, stream);
}

// (d_pixel_values, d_time) <- J^T d_prediction at the inputs of the last scot_plan_run (include/scot_plan.h).  Every refusal comes before
// the first copy: a refused call launches nothing and leaves the state as it was.
extern "C" int scot_plan_vjp(void* plan, const float* d_prediction, float* d_pixel_values, float* d_time, float grad_scale, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  if (pl->format != SCOT_PLAN_FORMAT_ADJOINT) return SCOT_ERR_UNSUPPORTED;
  const uint64_t* a = pl->adj;
  if (!d_prediction) return SCOT_ERR_SHAPE;
  if ((d_pixel_values && !(a[SCOT_PLAN_ADJ_FLAGS] & 1)) || (d_time && !(a[SCOT_PLAN_ADJ_FLAGS] & 2))) return SCOT_ERR_SHAPE;
  int exponent = 0;
  if (!scale_exponent(pl, grad_scale, &exponent)) return SCOT_ERR_SHAPE;
  if (!pl->ran) return SCOT_ERR_SHAPE;
  pl->ran = false;      // one vjp per run: the backward reuses saved rows
  if (!dev_copy(span_ptr(pl, pl->adj, SCOT_PLAN_ADJ_COT), d_prediction, (size_t)a[SCOT_PLAN_ADJ_COT + 2], D2D, stream)) return SCOT_ERR_LAUNCH;
  if (!write_scale(pl, exponent, stream)) return SCOT_ERR_LAUNCH;
  const int rc = replay(pl, SCOT_PLAN_CALLS_BACKWARD, stream);
  if (rc != SCOT_OK) return rc;
  if (d_pixel_values && !dev_copy(d_pixel_values, span_ptr(pl, pl->adj, SCOT_PLAN_ADJ_DPV), (size_t)a[SCOT_PLAN_ADJ_DPV + 2], D2D, stream)) return SCOT_ERR_LAUNCH;
  if (d_time && !dev_copy(d_time, span_ptr(pl, pl->adj, SCOT_PLAN_ADJ_DTIME), (size_t)a[SCOT_PLAN_ADJ_DTIME + 2], D2D, stream)) return SCOT_ERR_LAUNCH;
  return SCOT_OK;
}

// out[2]: non-finite values the un-scale passes have counted since load, the scale of the last vjp as an exponent.  Waits for `stream`.
extern "C" int scot_plan_grad_status(void* plan, long long* out, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl || !out) return SCOT_ERR_SHAPE;
  out[0] = out[1] = 0;
  if (pl->format != SCOT_PLAN_FORMAT_ADJOINT) return SCOT_ERR_UNSUPPORTED;
  int count = 0;
  if (pl->adj[SCOT_PLAN_ADJ_STATE + 2] && !dev_copy(&count, span_ptr(pl, pl->adj, SCOT_PLAN_ADJ_COUNTER), sizeof(count), D2H, stream)) return SCOT_ERR_LAUNCH;
  if (!dev_sync(stream)) return SCOT_ERR_LAUNCH;      // (also without a counter: the caller's gradients are complete on return)
  out[0] = count;
  out[1] = pl->last_exponent;
  return SCOT_OK;
}

// pl->host_time <- time / steps, read on the host (waits for `stream`).  torch's own rounding, so that the rollout equals harness.rollout
// bit for bit: torch's GPU kernel multiplies by the reciprocal of a host scalar (one rounding more than a division); its CPU kernel, which
// the emulated build is compared with, divides
static bool read_step_time(Plan* pl, const float* time, int steps, hipStream_t stream) {
  const size_t B = (size_t)pl->io[SCOT_PLAN_IO_B];
  try {
    pl->host_time.resize(B);
  } catch (const std::bad_alloc&) {
    return false;
  }
  if (!dev_copy(pl->host_time.data(), time, B * 4, D2H, stream) || !dev_sync(stream)) return false;
#ifdef SCOT_HIPEMU
  for (size_t b = 0; b < B; ++b) pl->host_time[b] = pl->host_time[b] / (float)steps;
#else
  const float inv_steps = 1.0f / (float)steps;
  for (size_t b = 0; b < B; ++b) pl->host_time[b] = pl->host_time[b] * inv_steps;
#endif
  return true;
}

// The integer form of the autoregressive rollout (reference trainer.py:452-603 with output_all_steps): time / steps once, then `steps`
// forwards, each prediction written to predictions[k] ([steps][B, Cout, H, W]) and copied back over the first Cout channels of the
// plan's input; the other input channels stay as given.  The division is the host's (one read of B floats: the call waits for
// `stream` once, before the first forward); everything after it is asynchronous.
extern "C" int scot_plan_rollout(void* plan, const float* pixel_values, const float* time, const void* pixel_mask, float* predictions,
                                 int steps, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  int rc = check_inputs(pl, pixel_values, time, pixel_mask, predictions);
  if (rc != SCOT_OK) return rc;
  const uint64_t* io = pl->io;
  if (steps < 1 || io[SCOT_PLAN_IO_COUT] > io[SCOT_PLAN_IO_CIN]) return SCOT_ERR_SHAPE;
  if (!io[SCOT_PLAN_IO_HAS_TIME]) return SCOT_ERR_UNSUPPORTED;      // (without conditioning the reference's rollout is one forward)
  pl->ran = false;      // (a rollout leaves nothing to differentiate: its forwards overwrite each other's saved rows)
  const size_t B = (size_t)io[SCOT_PLAN_IO_B], hw = (size_t)(io[SCOT_PLAN_IO_H] * io[SCOT_PLAN_IO_W] * 4);
  const size_t in_row = hw * io[SCOT_PLAN_IO_CIN], out_row = hw * io[SCOT_PLAN_IO_COUT];
  char* in = io_ptr(pl, SCOT_PLAN_IO_PV_BUF);
  char* out = io_ptr(pl, SCOT_PLAN_IO_OUT_BUF);
  if (!read_step_time(pl, time, steps, stream)) return SCOT_ERR_LAUNCH;
  if (!dev_copy(io_ptr(pl, SCOT_PLAN_IO_TIME_BUF), pl->host_time.data(), B * 4, H2D, stream)) return SCOT_ERR_LAUNCH;
  if (!copy_inputs(pl, pixel_values, nullptr, pixel_mask, stream)) return SCOT_ERR_LAUNCH;      // (time: the divided one, above)
  for (int k = 0; k < steps; ++k) {
    rc = replay(pl, SCOT_PLAN_CALLS_FORWARD, stream);
    if (rc != SCOT_OK) return rc;
    if (!dev_copy((char*)predictions + (size_t)k * B * out_row, out, B * out_row, D2D, stream)) return SCOT_ERR_LAUNCH;
    if (k + 1 < steps && !dev_copy2d(in, in_row, out, out_row, out_row, B, stream)) return SCOT_ERR_LAUNCH;
  }
  // (host_time is pageable memory: the runtime has staged it by the time the copy call returned)
  return SCOT_OK;
}

// A forward (steps == 1: scot_plan_run's) or a whole rollout (steps > 1: scot_plan_rollout's chain) that leaves only error sums behind
// (include/scot_plan.h): after forward k, scot_error_sums reduces the plan's own output buffer against targets[k] into sums[k] on
// `stream` — behind the list's join on a two-stream plan, before the buffer is copied back.  predictions may be NULL: no prediction
// leaves the plan.  Every refusal, the workspace's allocation included, comes before the first copy.
static int plan_evaluate(void* plan, const float* pixel_values, const float* time, const float* targets, const unsigned char* pixel_mask,
                         int mask_full, int steps, const int* channel_slices, int groups, double* sums, float* predictions, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  const uint64_t* io = pl->io;
  if (!pixel_values || !targets || !sums || steps < 1) return SCOT_ERR_SHAPE;
  const int B = (int)io[SCOT_PLAN_IO_B], cout = (int)io[SCOT_PLAN_IO_COUT], HW = (int)(io[SCOT_PLAN_IO_H] * io[SCOT_PLAN_IO_W]);
  // (groups outside 1..32, slices not strictly ascending or beyond Cout: the kernel's own rule, asked of its workspace query)
  if (scot_error_sums_workspace_bytes(B, cout, HW, channel_slices, groups) == 0) return SCOT_ERR_SHAPE;
  // (overwriting under the mask leaves a consistent prediction only where the groups tile [0, Cout): the kernel's rule, asked here first)
  if (pixel_mask && channel_slices && (channel_slices[0] != 0 || channel_slices[groups] != cout)) return SCOT_ERR_SHAPE;
  // (a mask input of a TRAINING plan belongs to its step lists: the inference list replayed here does not read it)
  if (io[SCOT_PLAN_IO_HAS_MASK] && pl->format != SCOT_PLAN_FORMAT_TRAINING) return SCOT_ERR_UNSUPPORTED;
  if (steps > 1) {
    if (io[SCOT_PLAN_IO_COUT] > io[SCOT_PLAN_IO_CIN]) return SCOT_ERR_SHAPE;
    if (!io[SCOT_PLAN_IO_HAS_TIME]) return SCOT_ERR_UNSUPPORTED;
  }
  if ((io[SCOT_PLAN_IO_HAS_TIME] != 0) != (time != nullptr)) return SCOT_ERR_SHAPE;
  if (!pl->eval_ws) {
    // any grouping of Cout channels: a group adds at most one chunk per sample to the one-group count (32 bytes a chunk)
    const size_t bytes = scot_error_sums_workspace_bytes(B, cout, HW, nullptr, 1) + (size_t)B * 31 * 4 * sizeof(double);
    pl->eval_ws = dev_alloc(bytes);
    if (!pl->eval_ws) return SCOT_ERR_LAUNCH;
    pl->eval_ws_bytes = bytes;
  }
  pl->ran = false;      // (like a rollout, an evaluation leaves nothing to differentiate)
  const size_t out_row = (size_t)HW * 4 * (size_t)cout, in_row = (size_t)HW * 4 * (size_t)io[SCOT_PLAN_IO_CIN], per_step = (size_t)B * (size_t)groups * 4;
  char* in = io_ptr(pl, SCOT_PLAN_IO_PV_BUF);
  char* out = io_ptr(pl, SCOT_PLAN_IO_OUT_BUF);
  if (steps > 1) {
    if (!read_step_time(pl, time, steps, stream)) return SCOT_ERR_LAUNCH;
    if (!dev_copy(io_ptr(pl, SCOT_PLAN_IO_TIME_BUF), pl->host_time.data(), (size_t)B * 4, H2D, stream)) return SCOT_ERR_LAUNCH;
    time = nullptr;      // (the divided one, above)
  }
  if (!copy_inputs(pl, pixel_values, time, nullptr, stream)) return SCOT_ERR_LAUNCH;
  for (int k = 0; k < steps; ++k) {
    int rc = replay(pl, SCOT_PLAN_CALLS_FORWARD, stream);
    if (rc != SCOT_OK) return rc;
#ifdef SCOT_HIPEMU
    ++g_emu_issued;
#endif
    // (a NULL mask is scot_error_sums itself; with one, the labels are stored over the masked positions of `out` before it is copied)
    rc = scot_error_sums_masked((float*)out, (const float*)((const char*)targets + (size_t)k * B * out_row), pixel_mask, mask_full, 1, B, cout, HW,
                                channel_slices, groups, sums + (size_t)k * per_step, pl->eval_ws, pl->eval_ws_bytes, stream);
    if (rc != SCOT_OK) return rc;
    if (predictions && !dev_copy((char*)predictions + (size_t)k * B * out_row, out, B * out_row, D2D, stream)) return SCOT_ERR_LAUNCH;
    if (k + 1 < steps && !dev_copy2d(in, in_row, out, out_row, out_row, B, stream)) return SCOT_ERR_LAUNCH;
  }
  // (host_time is pageable memory: the runtime has staged it by the time the copy call returned)
  return SCOT_OK;
}

extern "C" int scot_plan_evaluate(void* plan, const float* pixel_values, const float* time, const float* targets, int steps,
                                  const int* channel_slices, int groups, double* sums, float* predictions, hipStream_t stream) {
  return plan_evaluate(plan, pixel_values, time, targets, nullptr, 0, steps, channel_slices, groups, sums, predictions, stream);
}

// scot_plan_evaluate with the reference's pixel_mask (include/scot_plan.h): pixel_mask is the CALLER's device bytes, [B, Cout] (mask_full
// == 0) or [B, Cout, H, W], the same for every step; after forward k the fused kernel stores targets[k] over the masked positions of the
// plan's output buffer while it forms the sums, so the sums are the masked ones, the next step's input carries the labels there, and
// `predictions` receives the overwritten predictions.  NULL: scot_plan_evaluate.
extern "C" int scot_plan_evaluate_masked(void* plan, const float* pixel_values, const float* time, const float* targets, const void* pixel_mask,
                                         int mask_full, int steps, const int* channel_slices, int groups, double* sums, float* predictions,
                                         hipStream_t stream) {
  return plan_evaluate(plan, pixel_values, time, targets, (const unsigned char*)pixel_mask, mask_full, steps, channel_slices, groups, sums,
                       predictions, stream);
}

// The adjoint of that rollout with no detach between the steps (include/scot_plan.h): the gradient of sum_k <d_predictions[k],
// predictions[k]> with respect to pixel_values and time.  A checkpointed sweep: the step inputs are the caller's predictions, nothing
// else is kept.  For k = steps-1 .. 0: the whole input of step k is written again (the plan's input buffers are not assumed to outlive a
// backward), the forward list recomputes the saved activations, the cotangent d_predictions[k] + carry is formed AFTER that forward and
// the gradients are moved to the holder right after the backward (the plan's cotangent / gradient buffers are not assumed to outlive a
// forward).  The holder is the caller's d_pixel_values / d_time, so the sums are formed in place, in the order the header fixes.
// Every refusal, the holder's allocation included, comes before the first copy.
extern "C" int scot_plan_rollout_vjp(void* plan, const float* pixel_values, const float* time, const float* predictions,
                                     const float* d_predictions, int steps, float* d_pixel_values, float* d_time, float grad_scale,
                                     hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  if (pl->format != SCOT_PLAN_FORMAT_ADJOINT) return SCOT_ERR_UNSUPPORTED;
  const uint64_t* io = pl->io;
  const uint64_t* a = pl->adj;
  if (!io[SCOT_PLAN_IO_HAS_TIME] || io[SCOT_PLAN_IO_HAS_MASK]) return SCOT_ERR_UNSUPPORTED;
  if (steps < 1 || io[SCOT_PLAN_IO_COUT] > io[SCOT_PLAN_IO_CIN]) return SCOT_ERR_SHAPE;
  if (!pixel_values || !time || !predictions || !d_predictions) return SCOT_ERR_SHAPE;
  const bool has_dpv = (a[SCOT_PLAN_ADJ_FLAGS] & 1) != 0, has_dt = (a[SCOT_PLAN_ADJ_FLAGS] & 2) != 0;
  if ((!has_dpv && (steps > 1 || d_pixel_values)) || (!has_dt && d_time)) return SCOT_ERR_SHAPE;
  int exponent = 0;
  if (!scale_exponent(pl, grad_scale, &exponent)) return SCOT_ERR_SHAPE;
  const size_t B = (size_t)io[SCOT_PLAN_IO_B], hw = (size_t)(io[SCOT_PLAN_IO_H] * io[SCOT_PLAN_IO_W]);
  const size_t cin = (size_t)io[SCOT_PLAN_IO_CIN], cout = (size_t)io[SCOT_PLAN_IO_COUT];
  const size_t in_row = hw * cin * 4, out_row = hw * cout * 4;      // bytes of one sample
  // the carry's holder: the caller's d_pixel_values, or (more than one step and none given) a buffer of the runtime's own
  float* hold = d_pixel_values;
  if (!hold && steps > 1) {
    if (!pl->holder) {
      pl->holder = (float*)dev_alloc(B * in_row);
      if (!pl->holder) return SCOT_ERR_LAUNCH;
      pl->holder_bytes = B * in_row;
    }
    hold = pl->holder;
  }
  pl->ran = false;      // (the sweep's forwards overwrite the saved rows of any earlier run, and its backwards use their own up)
  char* in = io_ptr(pl, SCOT_PLAN_IO_PV_BUF);
  char* t = io_ptr(pl, SCOT_PLAN_IO_TIME_BUF);
  float* cot = (float*)span_ptr(pl, pl->adj, SCOT_PLAN_ADJ_COT);
  const float* g_pv = has_dpv ? (const float*)span_ptr(pl, pl->adj, SCOT_PLAN_ADJ_DPV) : nullptr;
  const float* g_t = has_dt ? (const float*)span_ptr(pl, pl->adj, SCOT_PLAN_ADJ_DTIME) : nullptr;
  if (!read_step_time(pl, time, steps, stream)) return SCOT_ERR_LAUNCH;
  for (int k = steps - 1; k >= 0; --k) {
    // step k's input: cat(predictions[k-1], pixel_values[:, Cout:]) — pixel_values itself for step 0 — and time / steps
    if (k == 0) {
      if (!dev_copy(in, pixel_values, B * in_row, D2D, stream)) return SCOT_ERR_LAUNCH;
    } else {
      if (!dev_copy2d(in, in_row, (const char*)predictions + (size_t)(k - 1) * B * out_row, out_row, out_row, B, stream)) return SCOT_ERR_LAUNCH;
      if (cin > cout && !dev_copy2d(in + out_row, in_row, (const char*)pixel_values + out_row, in_row, in_row - out_row, B, stream))
        return SCOT_ERR_LAUNCH;
    }
    if (!dev_copy(t, pl->host_time.data(), B * 4, H2D, stream)) return SCOT_ERR_LAUNCH;
    int rc = replay(pl, SCOT_PLAN_CALLS_FORWARD, stream);
    if (rc != SCOT_OK) return rc;
    const float* d_pred = (const float*)((const char*)d_predictions + (size_t)k * B * out_row);
    if (k == steps - 1) {
      if (!dev_copy(cot, d_pred, B * out_row, D2D, stream)) return SCOT_ERR_LAUNCH;
    } else if (!dev_cotangent(cot, d_pred, hold, B, cin, cout, hw, stream)) {
      return SCOT_ERR_LAUNCH;
    }
    if (!write_scale(pl, exponent, stream)) return SCOT_ERR_LAUNCH;
    rc = replay(pl, SCOT_PLAN_CALLS_BACKWARD, stream);
    if (rc != SCOT_OK) return rc;
    if ((hold || d_time) && !dev_carry(hold, g_pv, d_time, g_t, B, cin, cout, hw, k == steps - 1, k == 0, steps, stream)) return SCOT_ERR_LAUNCH;
  }
  // (host_time and host_scale are pageable memory: the runtime has staged them by the time the copy calls returned)
  return SCOT_OK;
}

// ------------------------------------------------------------------ training plans (image format 4)
// out[8]: has training, parameter groups, floats in the arena, calls of one step, bytes of labels, bytes kept between the step's forward
// and its backward, whether the gradient scale is dynamic, the kind of the batch's pixel_mask (0 none, 1 channel [B, Cout], 2 element
// [B, Cout, H, W]).  Format-1/2 plan: all zeros, status 0.
extern "C" int scot_plan_describe_training(void* plan, long long* out) {
  Plan* pl = as_plan(plan);
  if (!pl || !out) return SCOT_ERR_SHAPE;
  memset(out, 0, 8 * sizeof(long long));
  if (pl->format != SCOT_PLAN_FORMAT_TRAINING) return SCOT_OK;
  const uint64_t* t = pl->train;
  out[0] = 1;
  out[1] = (long long)t[SCOT_PLAN_TR_GROUPS];
  out[2] = (long long)t[SCOT_PLAN_TR_ARENA_FLOATS];
  for (int c = SCOT_PLAN_CALLS_STEP_FORWARD; c <= SCOT_PLAN_CALLS_UPDATE; ++c) out[3] += (long long)pl->list[c].calls;
  out[4] = (long long)t[SCOT_PLAN_TR_LABELS + 2];
  out[5] = (long long)t[SCOT_PLAN_TR_KEPT_BYTES];
  out[6] = (long long)(t[SCOT_PLAN_TR_FLAGS] & 1);
  out[7] = (t[SCOT_PLAN_TR_FLAGS] & 2) ? ((t[SCOT_PLAN_TR_FLAGS] & 4) ? 2 : 1) : 0;      // the batch's pixel_mask: none, channel, element
  return SCOT_OK;
}

// the batch -> the plan's input copies (the caller has checked the pointers): the inputs, the labels, and the mask of a masked plan
static bool copy_batch_in(Plan* pl, const float* pixel_values, const float* time, const float* labels, const void* pixel_mask, hipStream_t stream) {
  return copy_inputs(pl, pixel_values, time, pixel_mask, stream) &&
         dev_copy(span_ptr(pl, pl->train, SCOT_PLAN_TR_LABELS), labels, (size_t)pl->train[SCOT_PLAN_TR_LABELS + 2], D2D, stream);
}

// a batch for a training plan: pixel_values, labels, time where the plan takes it, and pixel_mask exactly where the plan is a masked one
static int check_batch(Plan* pl, const void* pixel_values, const void* time, const void* labels, const void* pixel_mask) {
  if (pl->format != SCOT_PLAN_FORMAT_TRAINING) return SCOT_ERR_UNSUPPORTED;
  if ((pl->io[SCOT_PLAN_IO_HAS_MASK] != 0) != (pixel_mask != nullptr)) return SCOT_ERR_SHAPE;
  return check_inputs(pl, pixel_values, time, nullptr, labels, false);
}

// loss [1] <- what model(pixel_values, time, labels=labels, pixel_mask=pixel_mask).loss returns, prediction (may be NULL) <- its output
// (the labels at the masked positions): the step's forward alone.  No state buffer is written.  pixel_mask: device bytes of the plan's
// mask size on a masked plan, NULL on any other.
extern "C" int scot_plan_loss_masked(void* plan, const float* pixel_values, const float* time, const float* labels, const void* pixel_mask,
                                     float* loss, float* prediction, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  int rc = check_batch(pl, pixel_values, time, labels, pixel_mask);
  if (rc != SCOT_OK) return rc;
  if (!loss) return SCOT_ERR_SHAPE;
  if (!copy_batch_in(pl, pixel_values, time, labels, pixel_mask, stream)) return SCOT_ERR_LAUNCH;
  rc = replay(pl, SCOT_PLAN_CALLS_STEP_FORWARD, stream);
  if (rc != SCOT_OK) return rc;
  if (!dev_copy(loss, span_ptr(pl, pl->train, SCOT_PLAN_TR_LOSS), 4, D2D, stream)) return SCOT_ERR_LAUNCH;
  if (prediction && !dev_copy(prediction, span_ptr(pl, pl->train, SCOT_PLAN_TR_PRED), (size_t)pl->train[SCOT_PLAN_TR_PRED + 2], D2D, stream)) return SCOT_ERR_LAUNCH;
  return SCOT_OK;
}

// the unmasked batch: on a masked plan the mask is missing (-1)
extern "C" int scot_plan_loss(void* plan, const float* pixel_values, const float* time, const float* labels, float* loss, float* prediction,
                              hipStream_t stream) {
  return scot_plan_loss_masked(plan, pixel_values, time, labels, nullptr, loss, prediction, stream);
}

// One optimizer step on the batch: forward, loss, backward, update (include/scot_plan.h).  lr is HOST memory, read before the call
// returns: it goes into the plan's own array, which the recorded scot_adamw_step call reads when it is issued.
extern "C" int scot_plan_train_step_masked(void* plan, const float* pixel_values, const float* time, const float* labels, const void* pixel_mask,
                                           const float* lr, float* loss, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  int rc = check_batch(pl, pixel_values, time, labels, pixel_mask);
  if (rc != SCOT_OK) return rc;
  if (!lr || !pl->lr || pl->accum_open) return SCOT_ERR_SHAPE;      // (an open accumulation ends with scot_plan_apply)
  if (!copy_batch_in(pl, pixel_values, time, labels, pixel_mask, stream)) return SCOT_ERR_LAUNCH;
  memcpy(pl->lr, lr, (size_t)pl->train[SCOT_PLAN_TR_GROUPS] * sizeof(float));
  for (int s = 0; s < 3; ++s)
    if ((rc = replay(pl, SCOT_PLAN_CALLS_STEP_FORWARD + s, stream)) != SCOT_OK) return rc;
  if (loss && !dev_copy(loss, span_ptr(pl, pl->train, SCOT_PLAN_TR_LOSS), 4, D2D, stream)) return SCOT_ERR_LAUNCH;
  return SCOT_OK;
}

extern "C" int scot_plan_train_step(void* plan, const float* pixel_values, const float* time, const float* labels, const float* lr, float* loss,
                                    hipStream_t stream) {
  return scot_plan_train_step_masked(plan, pixel_values, time, labels, nullptr, lr, loss, stream);
}

// ---- gradient accumulation: the step cut between its backward and its update (include/scot_plan.h)
// scot_grad_accumulate on the plan's gradient arena (counted in the emulation's launch log)
static int accumulate_pass(Plan* pl, float* dst, const float* acc, const float* grad, float weight, hipStream_t stream) {
#ifdef SCOT_HIPEMU
  ++g_emu_issued;
#endif
  return scot_grad_accumulate(dst, acc, grad, pl->group_map, (size_t)pl->train[SCOT_PLAN_TR_ARENA_FLOATS], weight, stream);
}

// One micro-batch: forward and backward as scot_plan_train_step_masked runs them, then A = weight * g (first) or A += weight * g.
extern "C" int scot_plan_accumulate(void* plan, const float* pixel_values, const float* time, const float* labels, const void* pixel_mask,
                                    float weight, int first, float* loss, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  int rc = check_batch(pl, pixel_values, time, labels, pixel_mask);
  if (rc != SCOT_OK) return rc;
  if (!pl->grad_arena || !(fabsf(weight) <= 3.4028234e38f) || (!first && !pl->accum_open)) return SCOT_ERR_SHAPE;
  if (!pl->accum) {
    const size_t bytes = (size_t)pl->train[SCOT_PLAN_TR_ARENA_FLOATS] * sizeof(float);
    pl->accum = (float*)dev_alloc(bytes);
    if (!pl->accum) return SCOT_ERR_LAUNCH;
    pl->accum_bytes = bytes;
    pl->accum_poisoned = true;      // (whoever held the memory before: zeroed below)
  }
  if (pl->accum_poisoned) {
    if (!dev_fill(pl->accum, 0, pl->accum_bytes, stream)) return SCOT_ERR_LAUNCH;
    pl->accum_poisoned = false;
  }
  if (first) pl->accum_open = 0;
  if (!copy_batch_in(pl, pixel_values, time, labels, pixel_mask, stream)) return SCOT_ERR_LAUNCH;
  for (int s = 0; s < 2; ++s)
    if ((rc = replay(pl, SCOT_PLAN_CALLS_STEP_FORWARD + s, stream)) != SCOT_OK) return rc;
  if ((rc = accumulate_pass(pl, pl->accum, first ? nullptr : pl->accum, pl->grad_arena, weight, stream)) != SCOT_OK) return rc;
  ++pl->accum_open;
  if (loss && !dev_copy(loss, span_ptr(pl, pl->train, SCOT_PLAN_TR_LOSS), 4, D2D, stream)) return SCOT_ERR_LAUNCH;
  return SCOT_OK;
}

// The update from the accumulator: gradient arena <- A at the parameter positions, then the recorded update list, unchanged.
extern "C" int scot_plan_apply(void* plan, const float* lr, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  if (pl->format != SCOT_PLAN_FORMAT_TRAINING) return SCOT_ERR_UNSUPPORTED;
  if (!lr || !pl->lr || !pl->accum_open) return SCOT_ERR_SHAPE;
  memcpy(pl->lr, lr, (size_t)pl->train[SCOT_PLAN_TR_GROUPS] * sizeof(float));
  int rc = accumulate_pass(pl, pl->grad_arena, nullptr, pl->accum, 1.0f, stream);
  if (rc != SCOT_OK) return rc;
  pl->accum_open = 0;      // (the gradient arena holds the sum: whatever the update does, this accumulation is over)
  return replay(pl, SCOT_PLAN_CALLS_UPDATE, stream);
}

// which = 0: the gradient arena the update reads; 1: the accumulator (-1 until the first scot_plan_accumulate has allocated it)
extern "C" int scot_plan_gradients(void* plan, int which, float** ptr, size_t* floats) {
  Plan* pl = as_plan(plan);
  if (!pl || !ptr || !floats) return SCOT_ERR_SHAPE;
  if (pl->format != SCOT_PLAN_FORMAT_TRAINING) return SCOT_ERR_UNSUPPORTED;
  float* p = which == 0 ? pl->grad_arena : (which == 1 ? pl->accum : nullptr);
  if (!p) return SCOT_ERR_SHAPE;
  *ptr = p;
  *floats = (size_t)pl->train[SCOT_PLAN_TR_ARENA_FLOATS];
  return SCOT_OK;
}

// out[2]: micro-batches in the open accumulation (0: none is open), bytes of the accumulator (0 before it is allocated)
extern "C" int scot_plan_accumulation_status(void* plan, long long* out) {
  Plan* pl = as_plan(plan);
  if (!pl || !out) return SCOT_ERR_SHAPE;
  out[0] = out[1] = 0;
  if (pl->format != SCOT_PLAN_FORMAT_TRAINING) return SCOT_ERR_UNSUPPORTED;
  out[0] = pl->accum_open;
  out[1] = (long long)pl->accum_bytes;
  return SCOT_OK;
}

// out[6]: steps applied, steps skipped, gradient scale (1 where it is not dynamic), last gradient norm before clipping, last clip
// coefficient, non-finite values the un-scale passes have counted.  Waits for `stream`.
extern "C" int scot_plan_train_status(void* plan, double* out, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl || !out) return SCOT_ERR_SHAPE;
  memset(out, 0, 6 * sizeof(double));
  if (pl->format != SCOT_PLAN_FORMAT_TRAINING) return SCOT_ERR_UNSUPPORTED;
  int steps[2] = {0, 0}, counted = 0;
  float clip[3] = {0.0f, 0.0f, 0.0f}, scale[4] = {1.0f, 1.0f, 0.0f, 0.0f};
  const bool dyn = (pl->train[SCOT_PLAN_TR_FLAGS] & 1) != 0;
  if (!dev_copy(steps, span_ptr(pl, pl->train, SCOT_PLAN_TR_STEP_STATE), sizeof(steps), D2H, stream)) return SCOT_ERR_LAUNCH;
  if (!dev_copy(clip, span_ptr(pl, pl->train, SCOT_PLAN_TR_CLIP), sizeof(clip), D2H, stream)) return SCOT_ERR_LAUNCH;
  if (dyn && (!dev_copy(scale, span_ptr(pl, pl->train, SCOT_PLAN_TR_SCALE_STATE), sizeof(scale), D2H, stream) ||
              !dev_copy(&counted, span_ptr(pl, pl->train, SCOT_PLAN_TR_COUNTER), sizeof(counted), D2H, stream)))
    return SCOT_ERR_LAUNCH;
  if (!dev_sync(stream)) return SCOT_ERR_LAUNCH;
  out[0] = steps[0];
  out[1] = steps[1];
  out[2] = scale[0];
  out[3] = clip[1];
  out[4] = clip[0];
  out[5] = counted;
  return SCOT_OK;
}

// image <- the current value of every stored STATE buffer.  `image` is a host copy of the image this plan was loaded from: same size,
// header, buffer table and training words (anything else: -1, nothing copied).  Waits for `stream`.
extern "C" int scot_plan_snapshot(void* plan, void* image, size_t bytes, hipStream_t stream) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  if (pl->format != SCOT_PLAN_FORMAT_TRAINING) return SCOT_ERR_UNSUPPORTED;
  const uint64_t* h = pl->header;
  if (!image || bytes != (size_t)h[SCOT_PLAN_H_BYTES] || memcmp(image, h, sizeof(pl->header)) != 0) return SCOT_ERR_SHAPE;
  char* b = (char*)image;      // (the header is the loaded one's: every offset below was validated at load against this size)
  if (memcmp(b + h[SCOT_PLAN_H_BUFFERS_OFF], pl->buffer_table.data(), pl->buffer_table.size() * 8) != 0 ||
      memcmp(b + h[SCOT_PLAN_H_TRAIN_OFF], pl->train, sizeof(pl->train)) != 0)
    return SCOT_ERR_SHAPE;
  for (size_t i = 0; i < pl->buf.size(); ++i)
    if (pl->buf_kind[i] == SCOT_PLAN_BUF_STATE && pl->buffer_table[4 * i + 3] == 1 &&
        !dev_copy(b + h[SCOT_PLAN_H_DATA_OFF] + pl->buffer_table[4 * i + 2], pl->buf[i], (size_t)pl->buf_bytes[i], D2H, stream))
      return SCOT_ERR_LAUNCH;
  return dev_sync(stream) ? SCOT_OK : SCOT_ERR_LAUNCH;
}

// ------------------------------------------------------------------ two-stream plans (image formats 5 and 6)
// *overlaps <- 1 when `b` runs beside `a` under the engine's fork / join pattern (K1 on a; b waits for it; K2 on b beside K3 on a; a
// waits for K2: three spin kernels of ~0.5 ms in less than 2.5 kernel times, the best of two trials), 0 when the pair serialises or
// a == b.  Waits for both streams.  The CPU emulation answers 0.
extern "C" int scot_stream_overlaps(hipStream_t a, hipStream_t b, int* overlaps) {
  if (!overlaps) return SCOT_ERR_SHAPE;
  const int r = dev_overlaps(a, b);
  *overlaps = r == 1;
  return r < 0 ? SCOT_ERR_LAUNCH : SCOT_OK;
}

// the host's own side stream instead of the one the load picked: between the load and the first run.  -3 on a one-stream plan.
extern "C" int scot_plan_set_side_stream(void* plan, hipStream_t side) {
  Plan* pl = as_plan(plan);
  if (!pl) return SCOT_ERR_SHAPE;
  if (pl->n_streams < 2) return SCOT_ERR_UNSUPPORTED;
  if (pl->started || !side || side == pl->load_stream) return SCOT_ERR_SHAPE;
  const int measured = dev_overlaps(pl->load_stream, side);
  if (measured < 0) return SCOT_ERR_LAUNCH;
  if (pl->side_own) dev_stream_destroy(pl->side);
  pl->side = side;
  pl->side_own = false;
  pl->side_host = true;
  pl->side_overlaps = measured;
  return SCOT_OK;
}

// out[4]: streams (1 or 2), events, whether the side stream was measured to run beside the load's stream, whether it is the host's
extern "C" int scot_plan_describe_streams(void* plan, long long* out) {
  Plan* pl = as_plan(plan);
  if (!pl || !out) return SCOT_ERR_SHAPE;
  out[0] = (long long)pl->n_streams;
  out[1] = (long long)pl->events.size();
  out[2] = pl->side_overlaps;
  out[3] = pl->side_host;
  return SCOT_OK;
}

// A test aid, like scot_plan_poison: later calls issue list `list` (SCOT_PLAN_CALLS_*) entry by entry in `order` — a permutation of
// 0 .. n-1 over the list's n entries, anything else -1 — with both streams synchronised whenever the stream of the next entry differs from
// the previous one's, so that the device executes exactly that order.  order = NULL restores the normal replay.  Whether an order is
// LEGAL (respects stream order and the event edges) is for the caller to know: tests/tape_schedule.py derives the legal ones.
extern "C" int scot_plan_issue_order(void* plan, int list, const int* order, int n) {
  Plan* pl = as_plan(plan);
  if (!pl || list < 0 || list >= SCOT_PLAN_N_CALLS) return SCOT_ERR_SHAPE;
  Plan::Program& p = pl->list[list];
  if (!order) {
    p.order.clear();
    return SCOT_OK;
  }
  if (n < 0 || (uint64_t)n != p.calls || n == 0) return SCOT_ERR_SHAPE;
  try {
    std::vector<char> seen((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
      if (order[k] < 0 || order[k] >= n || seen[order[k]]) return SCOT_ERR_SHAPE;
      seen[order[k]] = 1;
    }
    p.order.assign(order, order + n);
  } catch (const std::bad_alloc&) {
    return SCOT_ERR_LAUNCH;
  }
  return SCOT_OK;
}
