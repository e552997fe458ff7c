// error_sums — what evaluation reduces a prediction to: per sample and per channel group, the four sums the reference's metrics are
// made of (reference scOT/metrics.py, scOT/inference.py compute_metrics), in one pass over (prediction, target).
//
//   sums[b][g] = { sum |p - t|, sum |t|, sum (p - t)^2, sum t^2 }   over channels [slices[g], slices[g+1]) and every pixel of sample b
//
// Declared in include/scot_plan.h (a stand-alone call of the model-level header, like scot_stream_overlaps): it is NOT an entry point of
// scot_hip.h, so the ABI number stands and no recorded call list of a plan image can name it.
//
// ORDER.  Every term and every sum is fp64 (both fp32 values are converted first, then subtracted).  In NCHW the elements of one
// (sample, group) are ONE contiguous run of (c1 - c0) * HW floats.  A run is cut into chunks of CHUNK floats — a compile-time constant,
// never a number derived from the device — and one workgroup reduces one chunk: lane t owns the floats 4t .. 4t+3 of each of the chunk's
// LOADS blocks of 1024 floats and adds their terms in ascending address order; the 256 lane sums meet in LDS (256 x 4 doubles = 8 KB) in a
// fixed tree (4, then 8, then 8 sequential adds) and four plain stores put the chunk's partials into the workspace.  A second launch adds a
// run's partials in chunk order.  No atomics anywhere: the result is bitwise the same from launch to launch, on any device, and — since a
// lane owns the same floats whether it fetches them as one 16-byte load or as four scalar ones — whatever the alignment of the operands.
// Inf and NaN go through: nothing is clamped, a non-finite input makes exactly the sums it enters non-finite.
//
// MEMORY.  HBM-bound: two reads, almost no writes.  A run whose start is 16-byte aligned in both operands and whose length is a multiple
// of 4 floats is read with float4 loads (the rule of vec4_ok in plan.hip, per run), any other with scalar loads.  The loads carry no
// guard: a whole chunk needs none, and a run's last, short chunk clamps the index into the run and masks the TERM instead (a guarded load
// compiles to an exec-masked block with a wait of its own, one load per operand in flight).  In the gfx950 code of a whole chunk the
// 2 x LOADS global_load_dwordx4 of a lane precede the first s_waitcnt, which then counts down from vmcnt(7).
//
// MASKED (scot_error_sums_masked).  The reference pins masked positions to the labels before any metric (scOT/model.py: prediction[mask]
// = labels[mask]); the masked form does that inside the same pass: a masked element enters every sum as if p were t — its term is still
// d = (double)t - (double)t, so a non-finite LABEL under the mask makes the same sums non-finite as in the overwritten tensor, while a
// non-finite PREDICTION under the mask reaches no sum — and, with `overwrite`, t is stored over p there.  The sums are bit for bit those of
// the unmasked kernel on where(mask, target, pred): the same chunks, the same lane ownership (a lane stores only floats it owns), the same
// LDS tree, the same second launch.  The kernel is ONE template: MODE 0 is the kernel above, untouched (its branch is the code it always
// was); MODE 1 reads a channel mask [B, C]: a chunk that lies inside one plane (every chunk where HW is a multiple of CHUNK, so all of a
// 128 x 128 preset's) reads ONE mask byte per workgroup and selects on it after the data loads — pred is read whatever the byte says: a
// skip of the masked planes' loads is a branch on loaded data in front of all loads (profiles/plan_eval/README.md §6); a chunk that spans
// planes finds each lane's first channel with one division per load (32-bit below 2^32 floats a run) and steps from there (small planes
// only; not timed).  The load path (float4 or scalar) follows the alignment of the pointers this instantiation really reads.  MODE 2
// reads an element mask [B, C, HW] at any byte alignment: on the vector path the four bytes of a lane's four floats are fetched with one
// 4-byte copy, which the compiler is free to make one unaligned 32-bit load.  The masked branch folds whole and short chunks into one
// path (clamped index, masked term), as the scalar branch of MODE 0 does.
#include "common.h"

namespace {
const int THREADS = 256;
const int LOADS = 4;                             // 16-byte loads per lane and operand
const int CHUNK = THREADS * 4 * LOADS;           // floats of a run one workgroup reduces: 4096
const int MAX_GROUPS = 32;

// the groups, by value in the kernel arguments (the host array is read before the call returns): the channel slices and, per group, the
// first chunk of its runs within a sample's chunks
struct Groups {
  int n;
  int slice[MAX_GROUPS + 1];
  unsigned first_chunk[MAX_GROUPS + 1];          // first_chunk[n] = chunks per sample
};

// false: bad shape, groups outside 1..32, slices not strictly ascending inside [0, C], or more chunks than a grid holds
bool plan_groups(int B, int C, int HW, const int* slices, int groups, Groups* out) {
  if (B < 1 || C < 1 || HW < 1 || groups < 1 || groups > MAX_GROUPS) return false;
  if (!slices && groups != 1) return false;
  out->n = groups;
  size_t chunks = 0;
  for (int g = 0; g <= groups; ++g) {
    const int s = slices ? slices[g] : (g == 0 ? 0 : C);
    if (s < 0 || s > C || (g > 0 && s <= out->slice[g - 1])) return false;
    out->slice[g] = s;
    if (g > 0) chunks += ((size_t)(s - out->slice[g - 1]) * (size_t)HW + CHUNK - 1) / CHUNK;
    if (chunks * (size_t)B >= ((size_t)1 << 31)) return false;
    out->first_chunk[g] = (unsigned)chunks;
  }
  return true;
}

struct Acc {
  double ad, at, sd, st;                         // sum |p - t|, sum |t|, sum (p - t)^2, sum t^2
};
__device__ __forceinline__ void add_term(Acc& a, float pf, float tf) {
  const double p = (double)pf, t = (double)tf, d = p - t;
  a.ad += fabs(d);
  a.at += fabs(t);
  a.sd += d * d;
  a.st += t * t;
}

// stage 1: workgroup = one chunk of one (sample, group) run -> partial[workgroup][4].  MODE 0: no mask (pred_rw, mask, overwrite and
// channels are not read); 1: mask [B, C]; 2: mask [B, C, HW] — then `pred` is NULL and not touched: the prediction is read (and, with
// overwrite, written) through pred_rw alone, and its alignment decides the load path
template <int MODE>
__global__ __launch_bounds__(256) void error_sums_chunk_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                               double* __restrict__ partial, size_t sample_floats, size_t hw, Groups gr,
                                                               float* pred_rw, const unsigned char* __restrict__ mask, int overwrite,
                                                               int channels) {
  __shared__ double red[4][THREADS];
  const unsigned per_sample = gr.first_chunk[gr.n];
  const unsigned b = blockIdx.x / per_sample, k = blockIdx.x - b * per_sample;
  int g = 0;
  while (k >= gr.first_chunk[g + 1]) ++g;        // (k < first_chunk[n]: ends inside the table)
  const size_t run = (size_t)b * sample_floats + (size_t)gr.slice[g] * hw;
  const size_t len = (size_t)(gr.slice[g + 1] - gr.slice[g]) * hw;
  const size_t at = (size_t)(k - gr.first_chunk[g]) * CHUNK;      // this chunk's first float within the run
  const float* p = MODE == 0 ? pred + run + at : nullptr;
  const float* t = target + run + at;
  const size_t left = len - at;                  // >= 1 float
  const unsigned tid = threadIdx.x;
  Acc a = {0.0, 0.0, 0.0, 0.0};
  // (the pointer THIS instantiation reaches the prediction through: the same rule, so the same path as the unmasked kernel's, for any
  // alignment of either operand)
  const float* pred_base = MODE == 0 ? pred : (const float*)pred_rw;
  const bool vec = len % 4 == 0 && ((((uintptr_t)(pred_base + run)) | ((uintptr_t)(target + run))) & 15) == 0;
  if constexpr (MODE != 0) {
    float* pw = pred_rw + run + at;                // (the only pointer this branch reaches pred through)
    const bool whole = left >= (size_t)CHUNK;
    // where the mask bytes of this chunk are: MODE 2 at the floats' own offsets; MODE 1 one byte per channel of the run, and `plane`
    // when the chunk lies inside ONE channel (then one byte decides for the workgroup)
    const unsigned char* mrow;
    bool plane = false, plane_masked = false;
    size_t nch = 1;
    // the plane of float x of the run; a run shorter than 2^32 floats (x + CHUNK stays below 2^33 — uniform) divides in 32 bits
    const bool narrow = (len + CHUNK) >> 32 == 0;
    auto plane_of = [&](size_t x) -> size_t { return narrow ? (size_t)((unsigned)x / (unsigned)hw) : x / hw; };
    if (MODE == 1) {
      nch = (size_t)(gr.slice[g + 1] - gr.slice[g]);
      mrow = mask + (size_t)b * (size_t)channels + (size_t)gr.slice[g];
      const size_t first = plane_of(at);
      plane = plane_of(at + (whole ? (size_t)CHUNK : left) - 1) == first;
      // (the byte is only SELECTED on, further down: pred is read whatever it says, so that the byte's latency hides behind the data
      // loads; skipping the pred loads of a masked plane would be a branch on loaded data in front of every workgroup's loads)
      if (plane) plane_masked = mrow[first] != 0;
    } else {
      mrow = mask + run + at;
    }
    // bit e <- float i + e of this chunk is masked (MODE 1 across planes; i + e may lie behind the run: the channel is clamped)
    auto channel_bits = [&](size_t i) -> unsigned {
      size_t q = plane_of(at + i), r = (at + i) - q * hw;
      unsigned bits = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bits |= (unsigned)(mrow[q < nch ? q : nch - 1] != 0) << e;
        if (++r == hw) r = 0, ++q;
      }
      return bits;
    };
    if (vec) {
      // (a multiple of 4 floats is left: a lane's float4 is inside the run or wholly behind it)
      float4 pv[LOADS], tv[LOADS];
      unsigned mb[LOADS];
      size_t at_j[LOADS];
      bool in[LOADS];
      const size_t last = left - 4;
#pragma unroll
      for (int j = 0; j < LOADS; ++j) {
        const size_t i = (size_t)j * (THREADS * 4) + 4 * tid;
        in[j] = whole || i < left;
        at_j[j] = in[j] ? i : last;
        tv[j] = *(const float4*)(t + at_j[j]);
      }
#pragma unroll
      for (int j = 0; j < LOADS; ++j) pv[j] = *(const float4*)(pw + at_j[j]);
#pragma unroll
      for (int j = 0; j < LOADS; ++j) {
        if (MODE == 2) {
          unsigned four;
          __builtin_memcpy(&four, mrow + at_j[j], 4);      // (any alignment; inside the mask: at_j + 4 <= left)
          mb[j] = (unsigned)((four & 0xffu) != 0) | (unsigned)((four & 0xff00u) != 0) << 1 | (unsigned)((four & 0xff0000u) != 0) << 2 |
                  (unsigned)((four & 0xff000000u) != 0) << 3;
        } else {
          mb[j] = plane ? (plane_masked ? 15u : 0u) : channel_bits(at_j[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < LOADS; ++j) {
        if (in[j]) {
          float4 w = pv[j];
          if (mb[j] & 1) w.x = tv[j].x;
          if (mb[j] & 2) w.y = tv[j].y;
          if (mb[j] & 4) w.z = tv[j].z;
          if (mb[j] & 8) w.w = tv[j].w;
          add_term(a, w.x, tv[j].x);
          add_term(a, w.y, tv[j].y);
          add_term(a, w.z, tv[j].z);
          add_term(a, w.w, tv[j].w);
          // (the lane's own four floats: the unmasked ones get the bits back that were loaded from them)
          if (overwrite && mb[j]) *(float4*)(pw + at_j[j]) = w;
        }
      }
    } else {
      float pv[LOADS][4], tv[LOADS][4];
      unsigned mb[LOADS];
      const size_t last = left - 1;
#pragma unroll
      for (int j = 0; j < LOADS; ++j) {
        const size_t i0 = (size_t)j * (THREADS * 4) + 4 * tid;
        mb[j] = MODE == 2 ? 0u : (plane ? (plane_masked ? 15u : 0u) : channel_bits(i0));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const size_t i = whole || i0 + e < left ? i0 + e : last;
          tv[j][e] = t[i];
          pv[j][e] = pw[i];
          if (MODE == 2) mb[j] |= (unsigned)(mrow[i] != 0) << e;
        }
      }
#pragma unroll
      for (int j = 0; j < LOADS; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const size_t i = (size_t)j * (THREADS * 4) + 4 * tid + e;
          if (whole || i < left) {
            const bool m = (mb[j] >> e) & 1;
            add_term(a, m ? tv[j][e] : pv[j][e], tv[j][e]);
            if (overwrite && m) pw[i] = tv[j][e];
          }
        }
    }
  } else
  // A whole chunk (every chunk of a run but its last) takes UNGUARDED loads: a guarded load is its own exec-masked block with its own
  // wait, which leaves one load per operand in flight instead of LOADS.  Both branches add the same terms in the same order.
  if (vec) {
    // (a multiple of 4 floats is left: a lane's float4 is inside the run or wholly behind it)
    float4 pv[LOADS], tv[LOADS];
    if (left >= (size_t)CHUNK) {
#pragma unroll
      for (int j = 0; j < LOADS; ++j) pv[j] = *(const float4*)(p + j * (THREADS * 4) + 4 * tid);
#pragma unroll
      for (int j = 0; j < LOADS; ++j) tv[j] = *(const float4*)(t + j * (THREADS * 4) + 4 * tid);
#ifndef SCOT_HIPEMU
      __builtin_amdgcn_sched_group_barrier(0x020, 2 * LOADS, 0);      // (the 2 x LOADS loads first: the scheduler sinks none below a wait)
#endif
#pragma unroll
      for (int j = 0; j < LOADS; ++j) {
        add_term(a, pv[j].x, tv[j].x);
        add_term(a, pv[j].y, tv[j].y);
        add_term(a, pv[j].z, tv[j].z);
        add_term(a, pv[j].w, tv[j].w);
      }
    } else {
      // the run's last chunk: the index is clamped into the run (unguarded loads again) and the term is masked
      const size_t last = left - 4;
      bool in[LOADS];
#pragma unroll
      for (int j = 0; j < LOADS; ++j) {
        const size_t i = (size_t)j * (THREADS * 4) + 4 * tid;
        in[j] = i < left;
        pv[j] = *(const float4*)(p + (in[j] ? i : last));
        tv[j] = *(const float4*)(t + (in[j] ? i : last));
      }
#pragma unroll
      for (int j = 0; j < LOADS; ++j) {
        if (in[j]) {
          add_term(a, pv[j].x, tv[j].x);
          add_term(a, pv[j].y, tv[j].y);
          add_term(a, pv[j].z, tv[j].z);
          add_term(a, pv[j].w, tv[j].w);
        }
      }
    }
  } else {
    float pv[LOADS][4], tv[LOADS][4];
    const size_t last = left - 1;      // (a short chunk clamps the index into the run and masks the term, as above)
    const bool whole = left >= (size_t)CHUNK;
#pragma unroll
    for (int j = 0; j < LOADS; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const size_t i = (size_t)j * (THREADS * 4) + 4 * tid + e;
        pv[j][e] = p[whole || i < left ? i : last];
        tv[j][e] = t[whole || i < left ? i : last];
      }
#pragma unroll
    for (int j = 0; j < LOADS; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (whole || (size_t)j * (THREADS * 4) + 4 * tid + e < left) add_term(a, pv[j][e], tv[j][e]);
  }
  red[0][tid] = a.ad;
  red[1][tid] = a.at;
  red[2][tid] = a.sd;
  red[3][tid] = a.st;
  __syncthreads();
  // thread (q, l) of 4 x 64 is the only reader and the only writer of the entries it folds, at every level: the tree works in place
  const unsigned q = tid >> 6, l = tid & 63;
  red[q][l] = ((red[q][l] + red[q][l + 64]) + red[q][l + 128]) + red[q][l + 192];
  __syncthreads();
  if (l < 8) {
    double s = red[q][8 * l];
#pragma unroll
    for (int i = 1; i < 8; ++i) s += red[q][8 * l + i];
    red[q][8 * l] = s;
  }
  __syncthreads();
  if (l == 0) {
    double s = red[q][0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s += red[q][8 * i];
    partial[(size_t)blockIdx.x * 4 + q] = s;
  }
}

// stage 2: workgroup = one (sample, group), lane q < 4 = one of its four sums: the run's partials in chunk order.  ONE lane adds a run's
// partials serially: that is the ordering rule, and cheap at the presets (at most 16 chunks per run at 128 x 128 x 4 channels).  A large
// plane makes it a long single-lane chain of dependent adds (1024 x 1024: 256 chunks per channel); nobody has measured that.
__global__ __launch_bounds__(64) void error_sums_finish_kernel(const double* __restrict__ partial, double* __restrict__ sums, Groups gr) {
  const unsigned q = threadIdx.x, r = blockIdx.x, b = r / (unsigned)gr.n, g = r - b * (unsigned)gr.n;
  if (q >= 4) return;
  const double* src = partial + ((size_t)b * gr.first_chunk[gr.n] + gr.first_chunk[g]) * 4 + q;
  const unsigned n = gr.first_chunk[g + 1] - gr.first_chunk[g];
  double s = src[0];
  for (unsigned k = 1; k < n; ++k) s += src[(size_t)k * 4];
  sums[(size_t)r * 4 + q] = s;
}
}  // namespace

// bytes of workspace scot_error_sums needs for these arguments (0: it would refuse them)
extern "C" size_t scot_error_sums_workspace_bytes(int B, int C, int HW, const int* channel_slices, int groups) {
  Groups gr;
  if (!plan_groups(B, C, HW, channel_slices, groups, &gr)) return 0;
  return (size_t)B * gr.first_chunk[gr.n] * 4 * sizeof(double);
}

// the two launches behind both calls.  mask NULL: MODE 0.  Every refusal comes before the first launch.
static int error_sums_launch(float* pred, const float* target, const unsigned char* mask, int mask_full, int overwrite, int B, int C, int HW,
                             const int* channel_slices, int groups, double* sums, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  Groups gr;
  if (!pred || !target || !sums || !plan_groups(B, C, HW, channel_slices, groups, &gr)) return SCOT_ERR_SHAPE;
  const size_t chunks = (size_t)B * gr.first_chunk[gr.n];
  if (!workspace || workspace_bytes < chunks * 4 * sizeof(double) || ((uintptr_t)workspace & 7) || ((uintptr_t)sums & 7)) return SCOT_ERR_SHAPE;
  // overwriting pred leaves a consistent tensor only where every channel is in some group (groups are adjacent: first slice 0, last C)
  if (mask && overwrite && (gr.slice[0] != 0 || gr.slice[gr.n] != C)) return SCOT_ERR_SHAPE;
  const dim3 grid((unsigned)chunks), block(THREADS);
  const size_t sample_floats = (size_t)C * (size_t)HW;
  if (!mask)
    hipLaunchKernelGGL(error_sums_chunk_kernel<0>, grid, block, 0, stream, (const float*)pred, target, (double*)workspace, sample_floats,
                       (size_t)HW, gr, (float*)nullptr, (const unsigned char*)nullptr, 0, C);
  else if (!mask_full)
    hipLaunchKernelGGL(error_sums_chunk_kernel<1>, grid, block, 0, stream, (const float*)nullptr, target, (double*)workspace, sample_floats,
                       (size_t)HW, gr, pred, mask, (int)(overwrite != 0), C);
  else
    hipLaunchKernelGGL(error_sums_chunk_kernel<2>, grid, block, 0, stream, (const float*)nullptr, target, (double*)workspace, sample_floats,
                       (size_t)HW, gr, pred, mask, (int)(overwrite != 0), C);
  // (B * groups <= chunks: a grid holds it)
  hipLaunchKernelGGL(error_sums_finish_kernel, dim3((unsigned)B * (unsigned)groups), dim3(64), 0, stream, (const double*)workspace, sums, gr);
  return scot_check_launch();
}

// sums [B][groups][4] (fp64, device) <- the error sums of pred against target (fp32 [B, C, HW], device).  channel_slices: HOST memory,
// groups + 1 strictly ascending ints in [0, C], read before the call returns; NULL with groups == 1: the one group [0, C).
extern "C" int scot_error_sums(const float* pred, const float* target, int B, int C, int HW, const int* channel_slices, int groups,
                               double* sums, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  return error_sums_launch((float*)pred, target, nullptr, 0, 0, B, C, HW, channel_slices, groups, sums, workspace, workspace_bytes, stream);
}

// The same sums of the prediction where(mask, target, pred), bit for bit, in the same pass (include/scot_plan.h).  mask: bytes, non-zero =
// masked, [B, C] (mask_full == 0) or [B, C, HW] (mask_full != 0), any alignment; NULL: scot_error_sums.  overwrite != 0: target is stored
// over pred at the masked positions (needs groups that tile [0, C): otherwise -1); overwrite == 0: pred is read only.
extern "C" int scot_error_sums_masked(float* pred, const float* target, const unsigned char* mask, int mask_full, int overwrite, int B, int C,
                                      int HW, const int* channel_slices, int groups, double* sums, void* workspace, size_t workspace_bytes,
                                      hipStream_t stream) {
  return error_sums_launch(pred, target, mask, mask_full, overwrite, B, C, HW, channel_slices, groups, sums, workspace, workspace_bytes, stream);
}
