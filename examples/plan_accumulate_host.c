/* plan_accumulate_host — fine-tuning an exported ScOT model from plain C with an effective batch of M recorded batches: gradient
 * accumulation, no Python, no torch.
 *
 *   hipcc -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include examples/plan_accumulate_host.c -o plan_accumulate_host -ldl
 *   ./plan_accumulate_host poseidon_amd/libscot_hip_f16.so train.plan batches.bin lr.bin snapshot.plan M
 *
 * train.plan, batches.bin and snapshot.plan as for plan_train_host.c; batches.bin holds N x M micro-batches, update by update.  lr.bin
 * holds N x groups raw fp32 learning rates, one set per UPDATE.  Every update is M calls of scot_plan_accumulate with weight 1 / M (the
 * mean over the effective batch) and one scot_plan_apply.  Prints the mean loss and the status of every update and writes the training
 * state back as snapshot.plan.
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
typedef int (*accumulate_fn)(scot_plan_t, const float*, const float*, const float*, const void*, float, int, float*, scot_stream_t);
typedef int (*apply_fn)(scot_plan_t, const float*, scot_stream_t);
typedef int (*gradients_fn)(scot_plan_t, int, float**, size_t*);
typedef int (*status_fn)(scot_plan_t, double*, scot_stream_t);
typedef int (*snapshot_fn)(scot_plan_t, void*, size_t, scot_stream_t);
typedef int (*free_fn)(scot_plan_t);

int main(int argc, char** argv) {
  if (argc != 7 || atoi(argv[6]) < 1) {
    fprintf(stderr, "usage: %s <libscot_hip[_f16].so> <training plan> <batches.bin> <lr.bin> <snapshot out> <micro-batches per update>\n", argv[0]);
    return 2;
  }
  const size_t micro = (size_t)atoi(argv[6]);
  void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!lib) {
    fprintf(stderr, "dlopen: %s\n", dlerror());
    return 1;
  }
  load_fn plan_load = (load_fn)dlsym(lib, "scot_plan_load");
  describe_fn plan_describe = (describe_fn)dlsym(lib, "scot_plan_describe");
  describe_fn plan_describe_training = (describe_fn)dlsym(lib, "scot_plan_describe_training");
  accumulate_fn plan_accumulate = (accumulate_fn)dlsym(lib, "scot_plan_accumulate");
  apply_fn plan_apply = (apply_fn)dlsym(lib, "scot_plan_apply");
  gradients_fn plan_gradients = (gradients_fn)dlsym(lib, "scot_plan_gradients");
  status_fn plan_train_status = (status_fn)dlsym(lib, "scot_plan_train_status");
  snapshot_fn plan_snapshot = (snapshot_fn)dlsym(lib, "scot_plan_snapshot");
  free_fn plan_free = (free_fn)dlsym(lib, "scot_plan_free");
  if (!plan_load || !plan_describe || !plan_describe_training || !plan_accumulate || !plan_apply || !plan_gradients || !plan_train_status ||
      !plan_snapshot || !plan_free) {
    fprintf(stderr, "%s does not export the gradient accumulation calls\n", argv[1]);
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
  if (!tr[0] || tr[7]) {
    fprintf(stderr, "%s is not an unmasked training plan (image format %lld)\n", argv[2], d[15]);
    return 1;
  }
  const size_t pv_bytes = (size_t)d[13], time_bytes = (size_t)d[6], label_bytes = (size_t)tr[4], groups = (size_t)tr[1];
  const size_t one = pv_bytes + time_bytes + label_bytes;
  const size_t updates = batch_bytes / (one * micro);
  printf("training plan: batch %lld x %zu micro-batches, %lld x %lld, %lld parameters in %zu groups, %lld calls per step\n", d[0], micro, d[2],
         d[3], tr[2], groups, tr[3]);
  if (!updates || batch_bytes != updates * micro * one || lr_bytes != updates * groups * sizeof(float)) {
    fprintf(stderr, "%s holds %zu bytes (an update is %zu), %s holds %zu (an update is %zu)\n", argv[3], batch_bytes, one * micro, argv[4],
            lr_bytes, groups * sizeof(float));
    return 1;
  }
  /* the batches live on the device, as they would in a solver that produces them there */
  char* dev = NULL;
  float* loss = NULL;
  float* host_loss = (float*)malloc(micro * sizeof(float));
  CHECK_HIP(hipMalloc((void**)&dev, batch_bytes));
  CHECK_HIP(hipMalloc((void**)&loss, micro * sizeof(float)));
  CHECK_HIP(hipMemcpyAsync(dev, batches, batch_bytes, hipMemcpyHostToDevice, stream));
  const float weight = 1.0f / (float)micro;
  for (size_t u = 0; u < updates; ++u) {
    for (size_t k = 0; k < micro; ++k) {
      const char* b = dev + (u * micro + k) * one;
      rc = plan_accumulate(plan, (const float*)b, time_bytes ? (const float*)(b + pv_bytes) : NULL, (const float*)(b + pv_bytes + time_bytes), NULL,
                           weight, k == 0, loss + k, (scot_stream_t)stream);
      if (rc != 0) {
        fprintf(stderr, "scot_plan_accumulate %zu.%zu: status %d\n", u, k, rc);
        return 1;
      }
    }
    /* A data-parallel host, one plan per GPU, sums the accumulators of all ranks HERE, in this stream's order, before the update:
     *   float* acc; size_t floats;
     *   plan_gradients(plan, 1, &acc, &floats);
     *   scot_dp_allreduce_bucket over acc[0 .. floats), with the weight above divided by the number of ranks (include/scot_hip.h).
     * Every rank then applies the same reduced gradient and takes the same skip decision.  Never run on more than one GPU. */
    float* acc = NULL;
    size_t floats = 0;
    if (plan_gradients(plan, 1, &acc, &floats) != 0 || !acc || floats != (size_t)tr[2]) {
      fprintf(stderr, "scot_plan_gradients: no accumulator\n");
      return 1;
    }
    rc = plan_apply(plan, lr + u * groups, (scot_stream_t)stream);
    if (rc != 0) {
      fprintf(stderr, "scot_plan_apply %zu: status %d\n", u, rc);
      return 1;
    }
    double st[6], mean = 0.0;
    rc = plan_train_status(plan, st, (scot_stream_t)stream); /* (waits for the update: a real loop would ask every N updates) */
    if (rc != 0) return 1;
    CHECK_HIP(hipMemcpy(host_loss, loss, micro * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < micro; ++k) mean += (double)host_loss[k] / (double)micro;
    printf("update %zu loss %.9g applied %.0f skipped %.0f scale %g grad_norm %.6g clip %.6g nonfinite %.0f\n", u, mean, st[0], st[1], st[2], st[3],
           st[4], st[5]);
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
  free(host_loss);
  free(image);
  free(batches);
  free(lr);
  return 0;
}
