/* plan_eval_host — a trained ScOT model EVALUATED from plain C: a whole autoregressive rollout reduced to error sums on the device,
 * no prediction buffer, no Python, no torch.
 *
 *   hipcc -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include examples/plan_eval_host.c -o plan_eval_host -ldl
 *   ./plan_eval_host poseidon_amd/libscot_hip_f16.so model.plan input.bin targets.bin steps [channel slices, e.g. 0,1,3,4]
 *
 * model.plan comes from `ScOT.export_plan(pixel_values, time=..., path="model.plan")` (any image format).  input.bin holds the raw fp32
 * values of pixel_values [B, C, H, W] followed by those of time [B] (if the plan has a time input); targets.bin holds the raw fp32
 * targets [steps][B, Cout, H, W].  scot_plan_evaluate runs with predictions == NULL: the only thing that leaves the device is
 * sums [steps][B][groups][4] of double = { sum |p - t|, sum |t|, sum (p - t)^2, sum t^2 }.  Printed per step and channel group: the mean
 * and the median over the samples of the relative L1 error in percent, (S1 / N1) * 100 with N1 == 0 replaced by 1e-10 — the
 * reference's relative_lp_error (its scOT/metrics.py) — one line each:
 *   step <k> group <g> mean_relative_l1_error <x> median_relative_l1_error <y>
 */
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/scot_plan.h"

#define CHECK_HIP(call)                                                          \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s failed: %s\n", #call, hipGetErrorString(e_));          \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

static void* read_file(const char* path, size_t* bytes) {
  FILE* f = fopen(path, "rb");
  if (!f) return NULL;
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  void* p = NULL;
  if (n < 0 || posix_memalign(&p, 64, n > 0 ? (size_t)n : 64) != 0) {
    fclose(f);
    return NULL;
  }
  if (fread(p, 1, (size_t)n, f) != (size_t)n) {
    free(p);
    p = NULL;
  }
  fclose(f);
  *bytes = (size_t)n;
  return p;
}

static int ascending(const void* a, const void* b) {
  const double x = *(const double*)a, y = *(const double*)b;
  return (x > y) - (x < y);
}

int main(int argc, char** argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: %s <libscot_hip[_f16].so> <plan file> <input.bin> <targets.bin> <steps> [channel slices: 0,1,3,4]\n", argv[0]);
    return 2;
  }
  const int steps = atoi(argv[5]);
  int slices[33], groups = 1;
  const int* slice_arg = NULL;
  if (argc > 6) {
    int n = 0;
    char* text = strdup(argv[6]);
    for (char* tok = strtok(text, ","); tok && n < 33; tok = strtok(NULL, ",")) slices[n++] = atoi(tok);
    free(text);
    if (n < 2) {
      fprintf(stderr, "channel slices: at least two numbers\n");
      return 2;
    }
    groups = n - 1;
    slice_arg = slices;
  }
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!lib) {
    fprintf(stderr, "dlopen: %s\n", dlerror());
    return 1;
  }
  int (*plan_load)(const void*, size_t, scot_plan_t*, scot_stream_t) = (int (*)(const void*, size_t, scot_plan_t*, scot_stream_t))dlsym(lib, "scot_plan_load");
  int (*plan_describe)(scot_plan_t, long long*) = (int (*)(scot_plan_t, long long*))dlsym(lib, "scot_plan_describe");
  int (*plan_evaluate)(scot_plan_t, const float*, const float*, const float*, int, const int*, int, double*, float*, scot_stream_t) =
      (int (*)(scot_plan_t, const float*, const float*, const float*, int, const int*, int, double*, float*, scot_stream_t))dlsym(lib, "scot_plan_evaluate");
  int (*plan_free)(scot_plan_t) = (int (*)(scot_plan_t))dlsym(lib, "scot_plan_free");
  if (!plan_load || !plan_describe || !plan_evaluate || !plan_free) {
    fprintf(stderr, "%s does not export the plan calls with scot_plan_evaluate (ABI 8)\n", argv[1]);
    return 1;
  }
  size_t image_bytes = 0, input_bytes = 0, target_bytes = 0;
  void* image = read_file(argv[2], &image_bytes);
  void* input = read_file(argv[3], &input_bytes);
  void* targets = read_file(argv[4], &target_bytes);
  if (!image || !input || !targets) {
    fprintf(stderr, "cannot read %s\n", !image ? argv[2] : (!input ? argv[3] : argv[4]));
    return 1;
  }
  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  scot_plan_t plan = NULL;
  int rc = plan_load(image, image_bytes, &plan, (scot_stream_t)stream);
  free(image); /* the plan holds its own copy of everything */
  if (rc != 0) {
    fprintf(stderr, "scot_plan_load: status %d\n", rc);
    return 1;
  }
  long long d[16];
  plan_describe(plan, d);
  const size_t pv_bytes = (size_t)d[13], time_bytes = (size_t)d[6], out_bytes = (size_t)d[14], B = (size_t)d[0];
  if (steps < 1 || input_bytes != pv_bytes + time_bytes || target_bytes != out_bytes * (size_t)steps) {
    fprintf(stderr, "the plan takes %zu bytes of input (+ %zu of time) and %zu of targets per step: got %zu and %zu for %d steps\n", pv_bytes,
            time_bytes, out_bytes, input_bytes, target_bytes, steps);
    return 1;
  }
  const size_t n_sums = (size_t)steps * B * (size_t)groups * 4;
  float *pv = NULL, *t = NULL, *tg = NULL;
  double* sums = NULL;
  CHECK_HIP(hipMalloc((void**)&pv, pv_bytes));
  CHECK_HIP(hipMalloc((void**)&tg, target_bytes));
  CHECK_HIP(hipMalloc((void**)&sums, n_sums * sizeof(double)));
  CHECK_HIP(hipMemcpyAsync(pv, input, pv_bytes, hipMemcpyHostToDevice, stream));
  CHECK_HIP(hipMemcpyAsync(tg, targets, target_bytes, hipMemcpyHostToDevice, stream));
  if (time_bytes) {
    CHECK_HIP(hipMalloc((void**)&t, time_bytes));
    CHECK_HIP(hipMemcpyAsync(t, (const char*)input + pv_bytes, time_bytes, hipMemcpyHostToDevice, stream));
  }
  /* predictions == NULL: nothing but the sums leaves the plan */
  rc = plan_evaluate(plan, pv, t, tg, steps, slice_arg, groups, sums, NULL, (scot_stream_t)stream);
  if (rc != 0) {
    fprintf(stderr, "scot_plan_evaluate: status %d\n", rc);
    return 1;
  }
  double* host = (double*)malloc(n_sums * sizeof(double));
  double* rel = (double*)malloc(B * sizeof(double));
  if (!host || !rel) return 1;
  CHECK_HIP(hipMemcpyAsync(host, sums, n_sums * sizeof(double), hipMemcpyDeviceToHost, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  plan_describe(plan, d);
  printf("plan: batch %lld, %lld -> %lld channels, %lld x %lld, %d steps, %d groups, %.1f MB of device memory\n", d[0], d[1], d[4], d[2], d[3], steps,
         groups, (double)d[11] / 1e6);
  for (int k = 0; k < steps; ++k)
    for (int g = 0; g < groups; ++g) {
      double mean = 0.0;
      for (size_t b = 0; b < B; ++b) {
        const double* s = host + (((size_t)k * B + b) * (size_t)groups + (size_t)g) * 4;
        rel[b] = s[0] / (s[1] == 0.0 ? 1e-10 : s[1]) * 100.0;
        mean += rel[b];
      }
      qsort(rel, B, sizeof(double), ascending);
      const double median = B % 2 ? rel[B / 2] : 0.5 * (rel[B / 2 - 1] + rel[B / 2]);
      printf("step %d group %d mean_relative_l1_error %.17g median_relative_l1_error %.17g\n", k, g, mean / (double)B, median);
    }
  plan_free(plan);
  CHECK_HIP(hipFree(pv));
  CHECK_HIP(hipFree(tg));
  CHECK_HIP(hipFree(sums));
  if (t) CHECK_HIP(hipFree(t));
  CHECK_HIP(hipStreamDestroy(stream));
  free(host);
  free(rel);
  free(input);
  free(targets);
  return 0;
}
