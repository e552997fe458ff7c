/* plan_rollout_adjoint_host — the adjoint of a trained ScOT model's autoregressive rollout from plain C: no Python, no torch.
 *
 *   hipcc -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include examples/plan_rollout_adjoint_host.c -o plan_rollout_adjoint_host -ldl
 *   ./plan_rollout_adjoint_host poseidon_amd/libscot_hip_f16.so model.plan steps input.bin cotangents.bin predictions.bin \
 *                               d_pixel_values.bin d_time.bin [grad_scale]
 *
 * model.plan comes from `ScOT.export_plan(pixel_values, time=..., path="model.plan", adjoint=("pixel_values", "time"))`.  input.bin holds
 * the raw fp32 values of pixel_values [B, C, H, W] followed by those of time [B] (the lead time of the WHOLE rollout); cotangents.bin those
 * of d_predictions [steps][B, Cout, H, W]: the gradient of the host's own objective with respect to every step's prediction, zeros where a
 * step is not observed.  predictions.bin receives the rollout [steps][B, Cout, H, W]; the other two files the gradient of
 * sum_k <d_predictions[k], predictions[k]> with respect to pixel_values and to time, through all steps (a gradient the plan was not
 * exported with leaves its file empty).  grad_scale: the power of two an fp16 plan's backward runs under (default 0: the export-time
 * value); if grad_status counts non-finite values, call again under a smaller one.
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

static int write_file(const char* path, const void* p, size_t bytes) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) {
    fprintf(stderr, "cannot write %s\n", path);
    return 1;
  }
  fclose(f);
  return 0;
}

typedef int (*load_fn)(const void*, size_t, scot_plan_t*, scot_stream_t);
typedef int (*describe_fn)(scot_plan_t, long long*);
typedef int (*rollout_fn)(scot_plan_t, const float*, const float*, const void*, float*, int, scot_stream_t);
typedef int (*rollout_vjp_fn)(scot_plan_t, const float*, const float*, const float*, const float*, int, float*, float*, float, scot_stream_t);
typedef int (*grad_status_fn)(scot_plan_t, long long*, scot_stream_t);
typedef int (*free_fn)(scot_plan_t);

int main(int argc, char** argv) {
  if (argc < 9) {
    fprintf(stderr, "usage: %s <libscot_hip[_f16].so> <plan file> <steps> <input.bin> <cotangents.bin> <predictions.bin> "
                    "<d_pixel_values.bin> <d_time.bin> [grad_scale]\n", argv[0]);
    return 2;
  }
  const int steps = atoi(argv[3]);
  const float grad_scale = argc > 9 ? (float)atof(argv[9]) : 0.0f;
  if (steps < 1 || steps > 4096) {
    fprintf(stderr, "steps: 1 .. 4096\n");
    return 2;
  }
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!lib) {
    fprintf(stderr, "dlopen: %s\n", dlerror());
    return 1;
  }
  load_fn plan_load = (load_fn)dlsym(lib, "scot_plan_load");
  describe_fn plan_describe = (describe_fn)dlsym(lib, "scot_plan_describe");
  describe_fn plan_describe_adjoint = (describe_fn)dlsym(lib, "scot_plan_describe_adjoint");
  rollout_fn plan_rollout = (rollout_fn)dlsym(lib, "scot_plan_rollout");
  rollout_vjp_fn plan_rollout_vjp = (rollout_vjp_fn)dlsym(lib, "scot_plan_rollout_vjp");
  grad_status_fn plan_grad_status = (grad_status_fn)dlsym(lib, "scot_plan_grad_status");
  free_fn plan_free = (free_fn)dlsym(lib, "scot_plan_free");
  if (!plan_load || !plan_describe || !plan_describe_adjoint || !plan_rollout || !plan_rollout_vjp || !plan_grad_status || !plan_free) {
    fprintf(stderr, "%s does not export the rollout adjoint of the plan calls\n", argv[1]);
    return 1;
  }
  size_t image_bytes = 0, input_bytes = 0, cot_bytes = 0;
  void* image = read_file(argv[2], &image_bytes);
  void* input = read_file(argv[4], &input_bytes);
  void* cot = read_file(argv[5], &cot_bytes);
  if (!image || !input || !cot) {
    fprintf(stderr, "cannot read %s\n", !image ? argv[2] : (!input ? argv[4] : argv[5]));
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
  long long d[16], a[8];
  plan_describe(plan, d);
  plan_describe_adjoint(plan, a);
  if (!a[0] || !a[1] || !d[5]) {
    fprintf(stderr, "%s cannot differentiate a rollout: export a time-conditioned model with adjoint=(\"pixel_values\", \"time\")\n", argv[2]);
    return 1;
  }
  const size_t pv_bytes = (size_t)d[13], time_bytes = (size_t)d[6], out_bytes = (size_t)d[14], all_bytes = out_bytes * (size_t)steps;
  printf("plan: batch %lld, %lld -> %lld channels, %lld x %lld, %lld + %lld recorded calls, %.1f MB of device memory; %d steps: %d forwards, "
         "then %d forwards + %d backwards for the adjoint\n", d[0], d[1], d[4], d[2], d[3], d[12], a[3], (double)d[11] / 1e6, steps, steps,
         steps, steps);
  if (input_bytes != pv_bytes + time_bytes || cot_bytes != all_bytes) {
    fprintf(stderr, "the plan takes %zu (+ %zu of time) input bytes and, for %d steps, cotangents of %zu bytes\n", pv_bytes, time_bytes, steps,
            all_bytes);
    return 1;
  }
  float *pv = NULL, *t = NULL, *preds = NULL, *g = NULL, *d_pv = NULL, *d_t = NULL;
  CHECK_HIP(hipMalloc((void**)&pv, pv_bytes));
  CHECK_HIP(hipMalloc((void**)&t, time_bytes));
  CHECK_HIP(hipMalloc((void**)&preds, all_bytes));
  CHECK_HIP(hipMalloc((void**)&g, all_bytes));
  CHECK_HIP(hipMalloc((void**)&d_pv, pv_bytes));
  if (a[2]) CHECK_HIP(hipMalloc((void**)&d_t, time_bytes));
  CHECK_HIP(hipMemcpyAsync(pv, input, pv_bytes, hipMemcpyHostToDevice, stream));
  CHECK_HIP(hipMemcpyAsync(t, (const char*)input + pv_bytes, time_bytes, hipMemcpyHostToDevice, stream));
  CHECK_HIP(hipMemcpyAsync(g, cot, all_bytes, hipMemcpyHostToDevice, stream));
  /* the forward rollout: its predictions are the step inputs the adjoint recomputes from */
  rc = plan_rollout(plan, pv, t, NULL, preds, steps, (scot_stream_t)stream);
  if (rc != 0) {
    fprintf(stderr, "scot_plan_rollout: status %d\n", rc);
    return 1;
  }
  /* (a host's own objective would read preds here and write its gradient into g) */
  rc = plan_rollout_vjp(plan, pv, t, preds, g, steps, d_pv, d_t, grad_scale, (scot_stream_t)stream);
  if (rc != 0) {
    fprintf(stderr, "scot_plan_rollout_vjp: status %d\n", rc);
    return 1;
  }
  const size_t host_bytes = all_bytes + pv_bytes + time_bytes;
  char* host = (char*)malloc(host_bytes);
  if (!host) return 1;
  CHECK_HIP(hipMemcpyAsync(host, preds, all_bytes, hipMemcpyDeviceToHost, stream));
  CHECK_HIP(hipMemcpyAsync(host + all_bytes, d_pv, pv_bytes, hipMemcpyDeviceToHost, stream));
  if (d_t) CHECK_HIP(hipMemcpyAsync(host + all_bytes + pv_bytes, d_t, time_bytes, hipMemcpyDeviceToHost, stream));
  long long status[2];
  rc = plan_grad_status(plan, status, (scot_stream_t)stream); /* waits for the stream */
  if (rc != 0) {
    fprintf(stderr, "scot_plan_grad_status: status %d\n", rc);
    return 1;
  }
  printf("grad_status: %lld non-finite values counted, gradient scale 2^%lld\n", status[0], status[1]);
  if (write_file(argv[6], host, all_bytes) || write_file(argv[7], host + all_bytes, pv_bytes) ||
      write_file(argv[8], host + all_bytes + pv_bytes, d_t ? time_bytes : 0))
    return 1;
  plan_free(plan);
  CHECK_HIP(hipFree(pv));
  CHECK_HIP(hipFree(t));
  CHECK_HIP(hipFree(preds));
  CHECK_HIP(hipFree(g));
  CHECK_HIP(hipFree(d_pv));
  if (d_t) CHECK_HIP(hipFree(d_t));
  CHECK_HIP(hipStreamDestroy(stream));
  free(host);
  free(input);
  free(cot);
  return 0;
}
