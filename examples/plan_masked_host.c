/* plan_masked_host — fine-tuning and scoring an exported ScOT model under the reference's pixel_mask, from plain C.
 *
 *   hipcc -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include examples/plan_masked_host.c -o plan_masked_host -ldl
 *   ./plan_masked_host poseidon_amd/libscot_hip_f16.so masked.plan batches.bin lr.bin targets.bin <rollout steps>
 *
 * masked.plan comes from `ScOT.export_plan(pixel_values, time=..., labels=..., pixel_mask=M, train=optimizer, path="masked.plan")` with a
 * CHANNEL mask M (bool [B, Cout]: the constant density and pressure planes of the reference's incompressible sets).  batches.bin holds K
 * batches one after the other: the raw fp32 values of pixel_values [B, C, H, W], time [B] and labels [B, Cout, H, W], then the B * Cout
 * mask bytes (non-zero = masked), padded to a multiple of 4 bytes; lr.bin holds K x groups raw fp32 learning rates.  After the K steps
 * the first batch's pixel_values and time start a rollout of <rollout steps> steps that is scored against targets.bin ([steps][B, Cout, H,
 * W], fp32) under the first batch's mask with scot_plan_evaluate_masked: the masked planes are pinned to the targets, in the sums and in
 * what the next step reads.  Prints every step's loss and, per rollout step and sample, the relative L1 error in percent.
 */
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>

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

typedef int (*load_fn)(const void*, size_t, scot_plan_t*, scot_stream_t);
typedef int (*describe_fn)(scot_plan_t, long long*);
typedef int (*step_fn)(scot_plan_t, const float*, const float*, const float*, const void*, const float*, float*, scot_stream_t);
typedef int (*evaluate_fn)(scot_plan_t, const float*, const float*, const float*, const void*, int, int, const int*, int, double*, float*,
                           scot_stream_t);
typedef int (*free_fn)(scot_plan_t);

int main(int argc, char** argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: %s <libscot_hip[_f16].so> <masked training plan> <batches.bin> <lr.bin> <targets.bin> <rollout steps>\n", argv[0]);
    return 2;
  }
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!lib) {
    fprintf(stderr, "dlopen: %s\n", dlerror());
    return 1;
  }
  load_fn plan_load = (load_fn)dlsym(lib, "scot_plan_load");
  describe_fn plan_describe = (describe_fn)dlsym(lib, "scot_plan_describe");
  describe_fn plan_describe_training = (describe_fn)dlsym(lib, "scot_plan_describe_training");
  step_fn plan_train_step_masked = (step_fn)dlsym(lib, "scot_plan_train_step_masked");
  evaluate_fn plan_evaluate_masked = (evaluate_fn)dlsym(lib, "scot_plan_evaluate_masked");
  free_fn plan_free = (free_fn)dlsym(lib, "scot_plan_free");
  if (!plan_load || !plan_describe || !plan_describe_training || !plan_train_step_masked || !plan_evaluate_masked || !plan_free) {
    fprintf(stderr, "%s does not export the masked plan calls\n", argv[1]);
    return 1;
  }
  const int rollout = atoi(argv[6]);
  size_t image_bytes = 0, batch_bytes = 0, lr_bytes = 0, target_bytes = 0;
  void* image = read_file(argv[2], &image_bytes);
  char* batches = (char*)read_file(argv[3], &batch_bytes);
  float* lr = (float*)read_file(argv[4], &lr_bytes);
  float* targets = (float*)read_file(argv[5], &target_bytes);
  if (!image || !batches || !lr || !targets || rollout < 1) {
    fprintf(stderr, "cannot read the inputs\n");
    return 1;
  }
  hipStream_t stream;
  CHECK_HIP(hipStreamCreate(&stream));
  scot_plan_t plan = NULL;
  int rc = plan_load(image, image_bytes, &plan, (scot_stream_t)stream);
  if (rc != 0) {
    fprintf(stderr, "scot_plan_load: status %d\n", rc);
    return 1;
  }
  long long d[16], tr[8];
  plan_describe(plan, d);
  plan_describe_training(plan, tr);
  if (!tr[0] || tr[7] != 1 || !d[5]) {
    fprintf(stderr, "%s is not a training plan with a channel mask and a time input (mask kind %lld)\n", argv[2], tr[7]);
    return 1;
  }
  const size_t B = (size_t)d[0], pv_bytes = (size_t)d[13], time_bytes = (size_t)d[6], label_bytes = (size_t)tr[4], groups = (size_t)tr[1];
  const size_t mask_bytes = ((size_t)d[8] + 3) / 4 * 4;
  const size_t one = pv_bytes + time_bytes + label_bytes + mask_bytes, steps = batch_bytes / one;
  if (!steps || batch_bytes != steps * one || lr_bytes != steps * groups * sizeof(float) || target_bytes != (size_t)rollout * label_bytes) {
    fprintf(stderr, "the files do not hold whole batches, one lr per group and step, and %d target steps\n", rollout);
    return 1;
  }
  char* dev = NULL;
  float *loss = NULL, *dev_targets = NULL;
  double* sums = NULL;
  CHECK_HIP(hipMalloc((void**)&dev, batch_bytes));
  CHECK_HIP(hipMalloc((void**)&loss, steps * sizeof(float)));
  CHECK_HIP(hipMalloc((void**)&dev_targets, target_bytes));
  CHECK_HIP(hipMalloc((void**)&sums, (size_t)rollout * B * 4 * sizeof(double)));
  CHECK_HIP(hipMemcpyAsync(dev, batches, batch_bytes, hipMemcpyHostToDevice, stream));
  CHECK_HIP(hipMemcpyAsync(dev_targets, targets, target_bytes, hipMemcpyHostToDevice, stream));
  for (size_t k = 0; k < steps; ++k) {      /* every batch brings its own mask */
    const char* b = dev + k * one;
    rc = plan_train_step_masked(plan, (const float*)b, (const float*)(b + pv_bytes), (const float*)(b + pv_bytes + time_bytes),
                                b + pv_bytes + time_bytes + label_bytes, lr + k * groups, loss + k, (scot_stream_t)stream);
    if (rc != 0) {
      fprintf(stderr, "scot_plan_train_step_masked %zu: status %d\n", k, rc);
      return 1;
    }
  }
  /* the rollout at the trained weights, scored under the mask: one group of all channels, no prediction leaves the plan */
  rc = plan_evaluate_masked(plan, (const float*)dev, (const float*)(dev + pv_bytes), dev_targets, dev + pv_bytes + time_bytes + label_bytes, 0,
                            rollout, NULL, 1, sums, NULL, (scot_stream_t)stream);
  if (rc != 0) {
    fprintf(stderr, "scot_plan_evaluate_masked: status %d\n", rc);
    return 1;
  }
  float* host_loss = (float*)malloc(steps * sizeof(float));
  double* host_sums = (double*)malloc((size_t)rollout * B * 4 * sizeof(double));
  if (!host_loss || !host_sums) return 1;
  CHECK_HIP(hipMemcpyAsync(host_loss, loss, steps * sizeof(float), hipMemcpyDeviceToHost, stream));
  CHECK_HIP(hipMemcpyAsync(host_sums, sums, (size_t)rollout * B * 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
  CHECK_HIP(hipStreamSynchronize(stream));
  for (size_t k = 0; k < steps; ++k) printf("step %zu loss %.9g\n", k, (double)host_loss[k]);
  for (int k = 0; k < rollout; ++k)
    for (size_t b = 0; b < B; ++b) {
      const double* s = host_sums + ((size_t)k * B + b) * 4;      /* S1, N1, S2, N2 */
      printf("rollout %d sample %zu relative_l1 %.17g\n", k, b, s[0] / (s[1] == 0.0 ? 1e-10 : s[1]) * 100.0);
    }
  plan_free(plan);
  CHECK_HIP(hipFree(dev));
  CHECK_HIP(hipFree(loss));
  CHECK_HIP(hipFree(dev_targets));
  CHECK_HIP(hipFree(sums));
  CHECK_HIP(hipStreamDestroy(stream));
  free(image), free(batches), free(lr), free(targets), free(host_loss), free(host_sums);
  return 0;
}
