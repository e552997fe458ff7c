/* plan_train_host — fine-tuning an exported ScOT model from plain C: no Python, no torch.
 *
 *   hipcc -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include examples/plan_train_host.c -o plan_train_host -ldl
 *   ./plan_train_host poseidon_amd/libscot_hip_f16.so train.plan batches.bin lr.bin snapshot.plan
 *
 * train.plan comes from `ScOT.export_plan(pixel_values, time=..., labels=..., train=optimizer, path="train.plan")`.  batches.bin holds
 * K batches one after the other, each the raw fp32 values of pixel_values [B, C, H, W], time [B] (if the plan has a time input) and
 * labels [B, Cout, H, W]; lr.bin holds K x groups raw fp32 learning rates, step by step, in the optimizer's group order: the schedule
 * is the host's.  Prints the loss and the status of every step and writes the training state back as snapshot.plan — a training
 * image again: load it to go on, or bring it back with `poseidon_amd.plan.load_training_state`.
 * The library is the build the plan was exported from (libscot_hip_f16.so for the default fp16 mode, which opens libscot_hip.so
 * beside it for the trunk products).
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

typedef int (*load_fn)(const void*, size_t, scot_plan_t*, scot_stream_t);
typedef int (*describe_fn)(scot_plan_t, long long*);
typedef int (*step_fn)(scot_plan_t, const float*, const float*, const float*, const float*, float*, scot_stream_t);
typedef int (*status_fn)(scot_plan_t, double*, scot_stream_t);
typedef int (*snapshot_fn)(scot_plan_t, void*, size_t, scot_stream_t);
typedef int (*free_fn)(scot_plan_t);

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s <libscot_hip[_f16].so> <training plan> <batches.bin> <lr.bin> <snapshot out>\n", argv[0]);
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
  step_fn plan_train_step = (step_fn)dlsym(lib, "scot_plan_train_step");
  status_fn plan_train_status = (status_fn)dlsym(lib, "scot_plan_train_status");
  snapshot_fn plan_snapshot = (snapshot_fn)dlsym(lib, "scot_plan_snapshot");
  free_fn plan_free = (free_fn)dlsym(lib, "scot_plan_free");
  if (!plan_load || !plan_describe || !plan_describe_training || !plan_train_step || !plan_train_status || !plan_snapshot || !plan_free) {
    fprintf(stderr, "%s does not export the training plan calls\n", argv[1]);
    return 1;
  }
  size_t image_bytes = 0, batch_bytes = 0, lr_bytes = 0;
  void* image = read_file(argv[2], &image_bytes);      /* kept: the snapshot is written back into it */
  char* batches = (char*)read_file(argv[3], &batch_bytes);
  float* lr = (float*)read_file(argv[4], &lr_bytes);
  if (!image || !batches || !lr) {
    fprintf(stderr, "cannot read %s\n", !image ? argv[2] : (!batches ? argv[3] : argv[4]));
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
  if (!tr[0]) {
    fprintf(stderr, "%s is not a training plan (image format %lld)\n", argv[2], d[15]);
    return 1;
  }
  const size_t pv_bytes = (size_t)d[13], time_bytes = (size_t)d[6], label_bytes = (size_t)tr[4], groups = (size_t)tr[1];
  const size_t one = pv_bytes + time_bytes + label_bytes;
  const size_t steps = batch_bytes / one;
  printf("training plan: batch %lld, %lld x %lld, %lld parameters in %zu groups, %lld calls per step, %.1f MB of device memory\n", d[0], d[2], d[3],
         tr[2], groups, tr[3], (double)d[11] / 1e6);
  if (!steps || batch_bytes != steps * one || lr_bytes != steps * groups * sizeof(float)) {
    fprintf(stderr, "%s holds %zu bytes (a batch is %zu), %s holds %zu (a step is %zu)\n", argv[3], batch_bytes, one, argv[4], lr_bytes,
            groups * sizeof(float));
    return 1;
  }
  /* the batches live on the device, as they would in a solver that produces them there */
  char* dev = NULL;
  float* loss = NULL;
  CHECK_HIP(hipMalloc((void**)&dev, batch_bytes));
  CHECK_HIP(hipMalloc((void**)&loss, steps * sizeof(float)));
  CHECK_HIP(hipMemcpyAsync(dev, batches, batch_bytes, hipMemcpyHostToDevice, stream));
  for (size_t k = 0; k < steps; ++k) {
    const char* b = dev + k * one;
    rc = plan_train_step(plan, (const float*)b, time_bytes ? (const float*)(b + pv_bytes) : NULL, (const float*)(b + pv_bytes + time_bytes),
                         lr + k * groups, loss + k, (scot_stream_t)stream);
    if (rc != 0) {
      fprintf(stderr, "scot_plan_train_step %zu: status %d\n", k, rc);
      return 1;
    }
    double st[6];
    float l = 0.0f;
    rc = plan_train_status(plan, st, (scot_stream_t)stream); /* (waits for the step: a real loop would ask every N steps) */
    if (rc != 0) return 1;
    CHECK_HIP(hipMemcpy(&l, loss + k, sizeof(float), hipMemcpyDeviceToHost));
    printf("step %zu loss %.9g applied %.0f skipped %.0f scale %g grad_norm %.6g clip %.6g nonfinite %.0f\n", k, (double)l, st[0], st[1], st[2],
           st[3], st[4], st[5]);
  }
  rc = plan_snapshot(plan, image, image_bytes, (scot_stream_t)stream);
  if (rc != 0) {
    fprintf(stderr, "scot_plan_snapshot: status %d\n", rc);
    return 1;
  }
  FILE* f = fopen(argv[5], "wb");
  if (!f || fwrite(image, 1, image_bytes, f) != image_bytes) {
    fprintf(stderr, "cannot write %s\n", argv[5]);
    return 1;
  }
  fclose(f);
  plan_free(plan);
  CHECK_HIP(hipFree(dev));
  CHECK_HIP(hipFree(loss));
  CHECK_HIP(hipStreamDestroy(stream));
  free(image);
  free(batches);
  free(lr);
  return 0;
}
