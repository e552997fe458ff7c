/* plan_host — a trained ScOT model run from plain C: no Python, no torch.
 *
 *   hipcc -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include examples/plan_host.c -o plan_host -ldl
 *   ./plan_host poseidon_amd/libscot_hip_f16.so model.plan input.bin prediction.bin [steps]
 *
 * model.plan comes from `ScOT.export_plan(pixel_values, time=..., path="model.plan")`.  input.bin holds the raw fp32 values of
 * pixel_values [B, C, H, W] followed by those of time [B] (if the plan has a time input); prediction.bin receives the raw fp32
 * prediction [B, Cout, H, W], or with `steps` the `steps` predictions of an autoregressive rollout, one after the other.
 * The library is the build the plan was exported from: libscot_hip_f16.so for the default fp16 mode (it opens libscot_hip.so, which
 * lies beside it, for the trunk products), libscot_hip.so for the fp32 / bf16 modes.
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

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s <libscot_hip[_f16].so> <plan file> <input.bin> <prediction.bin> [rollout steps]\n", argv[0]);
    return 2;
  }
  const int steps = argc > 5 ? atoi(argv[5]) : 0;
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!lib) {
    fprintf(stderr, "dlopen: %s\n", dlerror());
    return 1;
  }
  int (*plan_load)(const void*, size_t, scot_plan_t*, scot_stream_t) = (int (*)(const void*, size_t, scot_plan_t*, scot_stream_t))dlsym(lib, "scot_plan_load");
  int (*plan_describe)(scot_plan_t, long long*) = (int (*)(scot_plan_t, long long*))dlsym(lib, "scot_plan_describe");
  int (*plan_run)(scot_plan_t, const float*, const float*, const void*, float*, scot_stream_t) =
      (int (*)(scot_plan_t, const float*, const float*, const void*, float*, scot_stream_t))dlsym(lib, "scot_plan_run");
  int (*plan_rollout)(scot_plan_t, const float*, const float*, const void*, float*, int, scot_stream_t) =
      (int (*)(scot_plan_t, const float*, const float*, const void*, float*, int, scot_stream_t))dlsym(lib, "scot_plan_rollout");
  int (*plan_free)(scot_plan_t) = (int (*)(scot_plan_t))dlsym(lib, "scot_plan_free");
  if (!plan_load || !plan_describe || !plan_run || !plan_rollout || !plan_free) {
    fprintf(stderr, "%s does not export the plan calls (ABI 8)\n", argv[1]);
    return 1;
  }
  size_t image_bytes = 0, input_bytes = 0;
  void* image = read_file(argv[2], &image_bytes);
  void* input = read_file(argv[3], &input_bytes);
  if (!image || !input) {
    fprintf(stderr, "cannot read %s\n", image ? argv[3] : argv[2]);
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
  const size_t pv_bytes = (size_t)d[13], time_bytes = (size_t)d[6], out_bytes = (size_t)d[14];
  printf("plan: batch %lld, %lld -> %lld channels, %lld x %lld, %lld recorded calls, %.1f MB of device memory\n", d[0], d[1], d[4], d[2], d[3],
         d[12], (double)d[11] / 1e6);
  if (input_bytes != pv_bytes + time_bytes) {
    fprintf(stderr, "%s holds %zu bytes, the plan takes %zu (+ %zu of time)\n", argv[3], input_bytes, pv_bytes, time_bytes);
    return 1;
  }
  const size_t n_out = steps > 0 ? (size_t)steps : 1;
  float *pv = NULL, *t = NULL, *pred = NULL;
  CHECK_HIP(hipMalloc((void**)&pv, pv_bytes));
  CHECK_HIP(hipMalloc((void**)&pred, out_bytes * n_out));
  CHECK_HIP(hipMemcpyAsync(pv, input, pv_bytes, hipMemcpyHostToDevice, stream));
  if (time_bytes) {
    CHECK_HIP(hipMalloc((void**)&t, time_bytes));
    CHECK_HIP(hipMemcpyAsync(t, (const char*)input + pv_bytes, time_bytes, hipMemcpyHostToDevice, stream));
  }
  rc = steps > 0 ? plan_rollout(plan, pv, t, NULL, pred, steps, (scot_stream_t)stream) : plan_run(plan, pv, t, NULL, pred, (scot_stream_t)stream);
  if (rc != 0) {
    fprintf(stderr, "%s: status %d\n", steps > 0 ? "scot_plan_rollout" : "scot_plan_run", rc);
    return 1;
  }
  float* host = (float*)malloc(out_bytes * n_out);
  if (!host) return 1;
  CHECK_HIP(hipMemcpyAsync(host, pred, out_bytes * n_out, hipMemcpyDeviceToHost, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  FILE* f = fopen(argv[4], "wb");
  if (!f || fwrite(host, 1, out_bytes * n_out, f) != out_bytes * n_out) {
    fprintf(stderr, "cannot write %s\n", argv[4]);
    return 1;
  }
  fclose(f);
  plan_free(plan);
  CHECK_HIP(hipFree(pv));
  CHECK_HIP(hipFree(pred));
  if (t) CHECK_HIP(hipFree(t));
  CHECK_HIP(hipStreamDestroy(stream));
  free(host);
  free(input);
  return 0;
}
