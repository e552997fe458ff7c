// plan_image_check — the plan image validator (poseidon_amd/csrc/plan_image.h) on its own, on the CPU.
//
//   plan_image_check <abi> <operand format> <image file> <expected status> [<image file> <expected status> ...]
//
// Runs scot_plan_image_validate over every file and compares the status with the expected one; for an accepted image it also walks
// everything the validator promised is in bounds: the names, every call list, the arrays, the io / adjoint / training words, and the
// bytes of the constants and of the stored state.  Each file is read into a heap block of exactly its size, so a build with
// -fsanitize=address,undefined turns any read past a truncated image into an error.  Exit status 0 when every image got the expected
// answer.  The cases are the callers': tests/plan_support.py (check_images_stand_alone) builds this file with the host sanitizers and hands it
// the good and the corrupt images of every format — among them masked training images (training flag bits 1 and 2) whose flag and mask
// input, or whose mask bytes and mask kind, disagree (tests/test_plan_masked_emu_cpu.py).
#include <stdio.h>
#include <stdlib.h>

#include "plan_image.h"

static uint64_t walk(const scot_plan_view* v) {
  uint64_t sum = 0;
  for (uint64_t i = 0; i < v->n_names; ++i) sum += strlen((const char*)(v->names + i * SCOT_PLAN_NAME_BYTES));
  for (uint64_t i = 0; i < v->n_buffers; ++i) {      // what the image holds by value: constants, and the stored state of a training image
    const uint64_t* buf = v->buffers + 4 * i;
    if (buf[0] == SCOT_PLAN_BUF_CONSTANT || (v->train && buf[0] == SCOT_PLAN_BUF_STATE && buf[3] == 1))
      for (uint64_t k = 0; k < buf[1]; k += 64) sum += v->data[buf[2] + k];
  }
  for (int c = 0; c < SCOT_PLAN_N_CALLS; ++c)
    for (uint64_t w = 0; w < v->calls[c].n_words; ++w) sum += v->calls[c].words[w];
  for (uint64_t w = 0; w < v->arrays_words; ++w) sum += v->arrays[w];
  for (int w = 0; w < SCOT_PLAN_IO_WORDS; ++w) sum += v->io[w];
  for (int w = 0; v->adj && w < SCOT_PLAN_ADJ_WORDS; ++w) sum += v->adj[w];
  for (int w = 0; v->train && w < SCOT_PLAN_TRAIN_WORDS; ++w) sum += v->train[w];
  return sum;
}

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 3) % 2) {
    fprintf(stderr, "usage: %s <abi> <operand format> <image> <expected status> ...\n", argv[0]);
    return 2;
  }
  const int abi = atoi(argv[1]), fmt = atoi(argv[2]);
  int bad = 0, n = 0;
  for (int a = 3; a + 1 < argc; a += 2, ++n) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    void* image = malloc(size > 0 ? (size_t)size : 1);      // (malloc: 16-byte aligned, exactly `size` bytes addressable)
    if (!image || (size > 0 && fread(image, 1, (size_t)size, f) != (size_t)size)) {
      fprintf(stderr, "cannot read %s\n", argv[a]);
      return 2;
    }
    fclose(f);
    scot_plan_view v;
    const int rc = scot_plan_image_validate(image, (size_t)size, abi, fmt, &v);
    const int want = atoi(argv[a + 1]);
    uint64_t sum = 0;
    if (rc == SCOT_PLAN_OK) sum = walk(&v);
    printf("%s: status %d (expected %d) checksum %llu\n", argv[a], rc, want, (unsigned long long)sum);
    if (rc != want) ++bad;
    free(image);
  }
  printf("%d images checked, %d unexpected\n", n, bad);
  return bad ? 1 : 0;
}
