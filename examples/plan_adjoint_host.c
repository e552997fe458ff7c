/* plan_adjoint_host — a trained ScOT model and its adjoint from plain C: no Python, no torch.
 *
 *   hipcc -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include examples/plan_adjoint_host.c -o plan_adjoint_host -ldl
 *   ./plan_adjoint_host poseidon_amd/libscot_hip_f16.so model.plan input.bin cotangent.bin prediction.bin d_pixel_values.bin d_time.bin [grad_scale]
 *
 * model.plan comes from `ScOT.export_plan(pixel_values, time=..., path="model.plan", adjoint=("pixel_values", "time"))`.  input.bin holds
 * the raw fp32 values of pixel_values [B, C, H, W] followed by those of time [B]; cotangent.bin those of d_prediction [B, Cout, H, W]
 * (the gradient of the host's own objective with respect to the prediction).  The three output files receive the raw fp32 prediction
 * and J^T d_prediction: the gradients with respect to pixel_values and to time (a gradient the plan was not exported with leaves its
 * file empty).  grad_scale: the power of two an fp16 plan's backward runs under (default 0: the export-time value).
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

int main(int argc, char** argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: %s <libscot_hip[_f16].so> <plan file> <input.bin> <cotangent.bin> <prediction.bin> <d_pixel_values.bin> "
                    "<d_time.bin> [grad_scale]\n", argv[0]);
    return 2;
  }
  const float grad_scale = argc > 8 ? (float)atof(argv[8]) : 0.0f;
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!lib) {
    fprintf(stderr, "dlopen: %s\n", dlerror());
    return 1;
  }
  int (*plan_load)(const void*, size_t, scot_plan_t*, scot_stream_t) = (int (*)(const void*, size_t, scot_plan_t*, scot_stream_t))dlsym(lib, "scot_plan_load");
  int (*plan_describe)(scot_plan_t, long long*) = (int (*)(scot_plan_t, long long*))dlsym(lib, "scot_plan_describe");
  int (*plan_describe_adjoint)(scot_plan_t, long long*) = (int (*)(scot_plan_t, long long*))dlsym(lib, "scot_plan_describe_adjoint");
  int (*plan_run)(scot_plan_t, const float*, const float*, const void*, float*, scot_stream_t) =
      (int (*)(scot_plan_t, const float*, const float*, const void*, float*, scot_stream_t))dlsym(lib, "scot_plan_run");
  int (*plan_vjp)(scot_plan_t, const float*, float*, float*, float, scot_stream_t) =
      (int (*)(scot_plan_t, const float*, float*, float*, float, scot_stream_t))dlsym(lib, "scot_plan_vjp");
  int (*plan_grad_status)(scot_plan_t, long long*, scot_stream_t) = (int (*)(scot_plan_t, long long*, scot_stream_t))dlsym(lib, "scot_plan_grad_status");
  int (*plan_free)(scot_plan_t) = (int (*)(scot_plan_t))dlsym(lib, "scot_plan_free");
  if (!plan_load || !plan_describe || !plan_describe_adjoint || !plan_run || !plan_vjp || !plan_grad_status || !plan_free) {
    fprintf(stderr, "%s does not export the adjoint plan calls\n", argv[1]);
    return 1;
  }
  size_t image_bytes = 0, input_bytes = 0, cot_bytes = 0;
  void* image = read_file(argv[2], &image_bytes);
  void* input = read_file(argv[3], &input_bytes);
  void* cot = read_file(argv[4], &cot_bytes);
  if (!image || !input || !cot) {
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
  long long d[16], a[8];
  plan_describe(plan, d);
  plan_describe_adjoint(plan, a);
  if (!a[0]) {
    fprintf(stderr, "%s is an inference plan: export it with adjoint=(\"pixel_values\", \"time\")\n", argv[2]);
    return 1;
  }
  const size_t pv_bytes = (size_t)d[13], time_bytes = (size_t)d[6], out_bytes = (size_t)d[14];
  printf("plan: batch %lld, %lld -> %lld channels, %lld x %lld, %lld + %lld recorded calls, %.1f MB of device memory, %.1f MB kept between "
         "run and vjp, default gradient scale 2^%lld\n", d[0], d[1], d[4], d[2], d[3], d[12], a[3], (double)d[11] / 1e6, (double)a[4] / 1e6, a[5]);
  if (input_bytes != pv_bytes + time_bytes || cot_bytes != out_bytes) {
    fprintf(stderr, "the plan takes %zu (+ %zu of time) input bytes and a cotangent of %zu bytes\n", pv_bytes, time_bytes, out_bytes);
    return 1;
  }
  float *pv = NULL, *t = NULL, *pred = NULL, *g = NULL, *d_pv = NULL, *d_t = NULL;
  CHECK_HIP(hipMalloc((void**)&pv, pv_bytes));
  CHECK_HIP(hipMalloc((void**)&pred, out_bytes));
  CHECK_HIP(hipMalloc((void**)&g, out_bytes));
  CHECK_HIP(hipMemcpyAsync(pv, input, pv_bytes, hipMemcpyHostToDevice, stream));
  CHECK_HIP(hipMemcpyAsync(g, cot, out_bytes, hipMemcpyHostToDevice, stream));
  if (time_bytes) {
    CHECK_HIP(hipMalloc((void**)&t, time_bytes));
    CHECK_HIP(hipMemcpyAsync(t, (const char*)input + pv_bytes, time_bytes, hipMemcpyHostToDevice, stream));
  }
  if (a[1]) CHECK_HIP(hipMalloc((void**)&d_pv, pv_bytes));
  if (a[2]) CHECK_HIP(hipMalloc((void**)&d_t, time_bytes));
  rc = plan_run(plan, pv, t, NULL, pred, (scot_stream_t)stream);
  if (rc != 0) {
    fprintf(stderr, "scot_plan_run: status %d\n", rc);
    return 1;
  }
  rc = plan_vjp(plan, g, d_pv, d_t, grad_scale, (scot_stream_t)stream);
  if (rc != 0) {
    fprintf(stderr, "scot_plan_vjp: status %d\n", rc);
    return 1;
  }
  const size_t host_bytes = out_bytes + pv_bytes + time_bytes;
  char* host = (char*)malloc(host_bytes ? host_bytes : 1);
  if (!host) return 1;
  CHECK_HIP(hipMemcpyAsync(host, pred, out_bytes, hipMemcpyDeviceToHost, stream));
  if (d_pv) CHECK_HIP(hipMemcpyAsync(host + out_bytes, d_pv, pv_bytes, hipMemcpyDeviceToHost, stream));
  if (d_t) CHECK_HIP(hipMemcpyAsync(host + out_bytes + pv_bytes, d_t, time_bytes, hipMemcpyDeviceToHost, stream));
  long long status[2];
  rc = plan_grad_status(plan, status, (scot_stream_t)stream); /* waits for the stream */
  if (rc != 0) {
    fprintf(stderr, "scot_plan_grad_status: status %d\n", rc);
    return 1;
  }
  printf("grad_status: %lld non-finite values counted, gradient scale 2^%lld\n", status[0], status[1]);
  if (write_file(argv[5], host, out_bytes) || write_file(argv[6], host + out_bytes, d_pv ? pv_bytes : 0) ||
      write_file(argv[7], host + out_bytes + pv_bytes, d_t ? time_bytes : 0))
    return 1;
  plan_free(plan);
  CHECK_HIP(hipFree(pv));
  CHECK_HIP(hipFree(pred));
  CHECK_HIP(hipFree(g));
  if (t) CHECK_HIP(hipFree(t));
  if (d_pv) CHECK_HIP(hipFree(d_pv));
  if (d_t) CHECK_HIP(hipFree(d_t));
  CHECK_HIP(hipStreamDestroy(stream));
  free(host);
  free(input);
  free(cot);
  return 0;
}
