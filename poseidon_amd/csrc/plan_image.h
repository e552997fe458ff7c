// plan_image — the format of an exported plan and its validator.  Header-only and HIP-free: plan.hip uses it inside the library,
// tools/plan_image_check.cc compiles it alone (with the host sanitizers) and runs it over good and corrupt images.
//
// A plan image (poseidon_amd/plan.py writes it) is a recording of the engine for one input signature, made relocatable: up to FIVE
// flat lists of C-ABI calls with their final arguments, every device address replaced by (buffer index, byte offset) and every stream
// argument by a placeholder.  All fields are little-endian uint64 words; the file is
//
//   header   SCOT_PLAN_HEADER_WORDS words (indices below)
//   names    n_names records of SCOT_PLAN_NAME_BYTES bytes: NUL-terminated entry-point names
//   buffers  n_buffers records of 4 words: kind, bytes, offset of the content in the data section (constants and stored state), 1 = a
//            STATE buffer stored by value (format 4).  STATE (formats 2 and 4) is device memory the RUNTIME writes: never poisoned,
//            zeroed at load unless stored — then uploaded at load, written by the steps, read back by scot_plan_snapshot
//   entries  the FORWARD list.  A list is variable-length records: name index, library (0 = the build that loads the image, 1 = the
//            bfloat16 build: the split-MFMA trunk GEMMs of the binary16 mode run there), n_int, n_flt, n_int argument pairs, n_flt
//            words of raw float bits (scot_plan_entry_words, scot_plan_entry_at)
//   arrays   n_arrays host arrays passed by address: kind (0 = int32, 1 = pointers, 2 = floats as raw bits in SCOT_PLAN_ARG_INT pairs,
//            format 4: the optimizer's per-group learning rates and weight decays), count, count argument pairs
//   io       SCOT_PLAN_IO_WORDS words: shapes and the (buffer, offset) of the inputs and of the prediction
//   lists    the other call lists of the format, each followed by the words that describe them (below)
//   data     the constants' and the stored state's bytes, each piece 64-byte aligned
//
// An argument pair is {tag | buffer << 8, value}: SCOT_PLAN_ARG_INT (value as is), _NULL, _PTR (buffer index, byte offset), _STREAM
// (value 0: the caller's stream at run time; value 1, formats 5 and 6: the plan's side stream), _ARRAY (value = index into `arrays`) or
// _EVENT (formats 5 and 6: value = index of one of the plan's events).
//
// TWO-STREAM images (`export_plan(..., streams=2)`): format 5 is a format-1 image, format 6 a format-4 image, whose lists hold the
// engine's own two-stream program: entries on stream 0 and stream 1 with the engine's fork and join edges as ordinary entries,
// scot_event_record (EVENT, STREAM) and scot_stream_wait_event (STREAM, EVENT) — the one more table of names, SCOT_PLAN_LIST_SYNC, which
// only these formats enable.  ONE header word (SCOT_PLAN_H_STREAMS_OFF) names the streams section: the number of streams (exactly 2) and
// the number of events.  Every list of such an image is CLOSED, and the validator holds it to that: a wait pairs with an earlier record
// of its event in the SAME list; the first entry on stream 1 is a wait for an event recorded on stream 0 of that list; the last entry on
// stream 1 is a record that stream 0 waits for further down.  So whatever runs in front of a list or behind it on stream 0 — the
// runtime's copies in and out, the next list, the caller's own work — is ordered with all of it, and the caller's contract stays "runs
// of one plan are ordered on the one stream you pass".  A library from before these formats refuses them by the format word (-3).
//
// RESIZED images (`export_plan(..., resize=True)` at a resolution r other than the model's) have no format, no section and no header word
// of their own: the forward list of a format-1, -2 or -5 image starts and ends with a scot_spectral_resize entry (a format-2 backward
// list likewise), the operator matrices are CONSTANT buffers, and the io words carry H = W = r.  A library from before that entry point
// refuses them by its name (-3).
//
// The five lists (SCOT_PLAN_CALLS_*), each held to ONE table of entry points (SCOT_PLAN_LIST_*): what can run is what is listed.
//
//   FORWARD        every format, table FORWARD: the inference forward.  In a format-2 image (an ADJOINT plan, `export_plan(...,
//                  adjoint=...)`) it is the DIFFERENTIABLE forward, which saves what the backward reads; in a format-4 image it is the
//                  plain inference forward, which reads the 16-bit copies the update keeps current
//   BACKWARD       format 2, table ADJOINT: the recorded vjp (cotangent of the prediction -> input gradients).  Named by header words
//                  the other formats leave zero, with the adjoint words: which gradients exist, the (buffer, offset, bytes) of the
//                  cotangent's copy, of d_pixel_values, of d_time, of the 16-byte gradient-scale state {S, 1/S, -, -} and of the
//                  non-finite counter of the un-scale passes, the export-time scale as a power-of-two exponent, the bytes a run leaves
//                  for the vjp
//   STEP_FORWARD, STEP_BACKWARD, UPDATE
//                  format 4 (a TRAINING plan, `export_plan(..., labels=..., train=optimizer)`; format 3 is unassigned), table
//                  TRAINING: the step's forward through the loss, its backward with the weight gradients (the zero fill of the
//                  accumulated gradients first, the un-scale passes last) and the optimizer update.  ONE header word names the
//                  training words, everything else is named from there: the (count, offset, words) of the three lists; the (buffer,
//                  offset, bytes) of the labels' copy, the loss and the step forward's prediction; the state spans (fp32 parameter
//                  arena, both moments, the 16-bit copies, the step counters, the three clip floats, the gradient-scale state and its
//                  non-finite counter); the number of parameter groups and the lr patch point: which argument of which update entry
//                  is the host array lr[groups] that scot_plan_train_step overwrites
#ifndef SCOT_PLAN_IMAGE_H
#define SCOT_PLAN_IMAGE_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define SCOT_PLAN_MAGIC 0x4e414c50544f4353ull /* "SCOTPLAN" */
#define SCOT_PLAN_FORMAT 1
#define SCOT_PLAN_FORMAT_ADJOINT 2
#define SCOT_PLAN_FORMAT_TRAINING 4 /* (3 is unassigned) */
#define SCOT_PLAN_FORMAT_STREAMS 5          /* format 1 + the streams section */
#define SCOT_PLAN_FORMAT_TRAINING_STREAMS 6 /* format 4 + the streams section */
#define SCOT_PLAN_STREAMS_WORDS 2
#define SCOT_PLAN_MAX_EVENTS 4096
#define SCOT_PLAN_HEADER_WORDS 32
#define SCOT_PLAN_NAME_BYTES 48
#define SCOT_PLAN_IO_WORDS 24
#define SCOT_PLAN_ADJ_WORDS 24
#define SCOT_PLAN_TRAIN_WORDS 64
#define SCOT_PLAN_ADAMW_LR_ARG 6 /* scot_adamw_step(params, grads, exp_avg, exp_avg_sq, map8, n, LR, wd, ...): the patch point */
#define SCOT_PLAN_MAX_INT 48 /* = SCOT_TAPE_MAX_INT of host_tape.hip: what one replayed call can carry */
#define SCOT_PLAN_MAX_FLT 8

/* a list is named by three consecutive words (count, offset in the image, words): H_NENTRIES.., H_NBACKWARD.., TR_FWD / _BWD / _UPD */
enum { SCOT_PLAN_H_MAGIC, SCOT_PLAN_H_FORMAT, SCOT_PLAN_H_ABI, SCOT_PLAN_H_OPERAND, SCOT_PLAN_H_COMPUTE, SCOT_PLAN_H_BYTES,
       SCOT_PLAN_H_NNAMES, SCOT_PLAN_H_NAMES_OFF, SCOT_PLAN_H_NBUFFERS, SCOT_PLAN_H_BUFFERS_OFF, SCOT_PLAN_H_NENTRIES,
       SCOT_PLAN_H_ENTRIES_OFF, SCOT_PLAN_H_ENTRIES_WORDS, SCOT_PLAN_H_NARRAYS, SCOT_PLAN_H_ARRAYS_OFF, SCOT_PLAN_H_ARRAYS_WORDS,
       SCOT_PLAN_H_IO_OFF, SCOT_PLAN_H_DATA_OFF, SCOT_PLAN_H_DATA_BYTES,
       /* format 2 */ SCOT_PLAN_H_NBACKWARD, SCOT_PLAN_H_BACKWARD_OFF, SCOT_PLAN_H_BACKWARD_WORDS, SCOT_PLAN_H_ADJ_OFF,
       /* format 4 */ SCOT_PLAN_H_TRAIN_OFF,
       /* formats 5, 6 */ SCOT_PLAN_H_STREAMS_OFF };
enum { SCOT_PLAN_ST_STREAMS, SCOT_PLAN_ST_EVENTS }; /* the streams section */
enum { SCOT_PLAN_BUF_CONSTANT, SCOT_PLAN_BUF_INPUT, SCOT_PLAN_BUF_OUTPUT, SCOT_PLAN_BUF_SCRATCH, SCOT_PLAN_BUF_STATE };
enum { SCOT_PLAN_ARG_INT, SCOT_PLAN_ARG_NULL, SCOT_PLAN_ARG_PTR, SCOT_PLAN_ARG_STREAM, SCOT_PLAN_ARG_ARRAY, SCOT_PLAN_ARG_EVENT };
enum { SCOT_PLAN_IO_B, SCOT_PLAN_IO_CIN, SCOT_PLAN_IO_H, SCOT_PLAN_IO_W, SCOT_PLAN_IO_COUT, SCOT_PLAN_IO_PV_BUF, SCOT_PLAN_IO_PV_OFF,
       SCOT_PLAN_IO_HAS_TIME, SCOT_PLAN_IO_TIME_BUF, SCOT_PLAN_IO_TIME_OFF, SCOT_PLAN_IO_TIME_BYTES, SCOT_PLAN_IO_HAS_MASK,
       SCOT_PLAN_IO_MASK_BUF, SCOT_PLAN_IO_MASK_OFF, SCOT_PLAN_IO_MASK_BYTES, SCOT_PLAN_IO_OUT_BUF, SCOT_PLAN_IO_OUT_OFF };
/* the adjoint words: FLAGS bit 0 = d_pixel_values, bit 1 = d_time; a span is (buffer, offset, bytes), bytes 0 = absent */
enum { SCOT_PLAN_ADJ_FLAGS, SCOT_PLAN_ADJ_COT, SCOT_PLAN_ADJ_DPV = SCOT_PLAN_ADJ_COT + 3, SCOT_PLAN_ADJ_DTIME = SCOT_PLAN_ADJ_DPV + 3,
       SCOT_PLAN_ADJ_STATE = SCOT_PLAN_ADJ_DTIME + 3, SCOT_PLAN_ADJ_COUNTER = SCOT_PLAN_ADJ_STATE + 3,
       SCOT_PLAN_ADJ_SCALE_EXP = SCOT_PLAN_ADJ_COUNTER + 3, SCOT_PLAN_ADJ_KEPT_BYTES };
/* the training words: FLAGS bit 0 = the gradient scale is dynamic (fp16), bit 1 = the batch has a pixel_mask (the io words name its
   input buffer, which the recorded scot_head_finalize / scot_loss_bwd entries read), bit 2 = it is an element mask [B, Cout, H, W] and
   not a channel mask [B, Cout] (a library from before the masks rejects FLAGS > 1: it cannot train unmasked on such an image); a span
   is (buffer, offset, bytes), bytes 0 = absent */
#define SCOT_PLAN_TR_FLAG_DYNAMIC 1
#define SCOT_PLAN_TR_FLAG_MASK 2
#define SCOT_PLAN_TR_FLAG_MASK_FULL 4
enum { SCOT_PLAN_TR_FLAGS, SCOT_PLAN_TR_GROUPS, SCOT_PLAN_TR_ARENA_FLOATS, SCOT_PLAN_TR_FWD, SCOT_PLAN_TR_BWD = SCOT_PLAN_TR_FWD + 3,
       SCOT_PLAN_TR_UPD = SCOT_PLAN_TR_BWD + 3, SCOT_PLAN_TR_LR_ENTRY = SCOT_PLAN_TR_UPD + 3, SCOT_PLAN_TR_LR_ARG, SCOT_PLAN_TR_KEPT_BYTES,
       SCOT_PLAN_TR_LABELS, SCOT_PLAN_TR_LOSS = SCOT_PLAN_TR_LABELS + 3, SCOT_PLAN_TR_PRED = SCOT_PLAN_TR_LOSS + 3,
       SCOT_PLAN_TR_ARENA = SCOT_PLAN_TR_PRED + 3, SCOT_PLAN_TR_EXP_AVG = SCOT_PLAN_TR_ARENA + 3,
       SCOT_PLAN_TR_EXP_AVG_SQ = SCOT_PLAN_TR_EXP_AVG + 3, SCOT_PLAN_TR_SHADOW = SCOT_PLAN_TR_EXP_AVG_SQ + 3,
       SCOT_PLAN_TR_SHADOW_T = SCOT_PLAN_TR_SHADOW + 3, SCOT_PLAN_TR_STEP_STATE = SCOT_PLAN_TR_SHADOW_T + 3,
       SCOT_PLAN_TR_CLIP = SCOT_PLAN_TR_STEP_STATE + 3, SCOT_PLAN_TR_SCALE_STATE = SCOT_PLAN_TR_CLIP + 3,
       SCOT_PLAN_TR_COUNTER = SCOT_PLAN_TR_SCALE_STATE + 3, SCOT_PLAN_TR_END = SCOT_PLAN_TR_COUNTER + 3 };

// What a forward may call.  (X-macros: plan.hip builds the table of addresses from them.)
#define SCOT_PLAN_ENTRY_POINTS(X)                                                                                                     \
  X(scot_gemm) X(scot_cpb_fwd_batched) X(scot_cln_fwd) X(scot_window_attn_fwd) X(scot_mlp_block_fwd) X(scot_block_tail_fwd)          \
  X(scot_proj_cln_fwd) X(scot_add) X(scot_copy2d) X(scot_space_to_depth) X(scot_depth_to_space) X(scot_patchify) X(scot_unpatchify) \
  X(scot_scale_residual) X(scot_dwconv7) X(scot_conv5) X(scot_head_finalize) X(scot_memset_async) X(scot_memcpy_async)              \
  X(scot_spectral_resize)

// What the backward of an adjoint plan may call: the data-gradient chain of the frozen model and nothing else — no weight-gradient
// kernel, no column sum into a parameter gradient, no optimizer step is listed in either table.
#define SCOT_PLAN_ADJOINT_ENTRY_POINTS(X)                                                                                            \
  X(scot_gemm) X(scot_cln_bwd) X(scot_cln_dtime) X(scot_window_attn_bwd_rep) X(scot_block_tail_bwd) X(scot_proj_cln_bwd) X(scot_add)  \
  X(scot_add_channels) X(scot_copy2d) X(scot_space_to_depth) X(scot_depth_to_space) X(scot_patchify) X(scot_unpatchify)              \
  X(scot_scale_residual) X(scot_dwconv7) X(scot_conv5) X(scot_scale_inplace_dev) X(scot_pow2_rescale) X(scot_colscale_dev)           \
  X(scot_axpy_dev) X(scot_memset_async) X(scot_memcpy_async) X(scot_spectral_resize)

// What the three step lists of a training plan may call: the differentiable forward with the loss, the whole backward — data AND
// weight gradients —, the gradient arena's fill and un-scale, and the optimizer update.  A table of its own: none of the weight-gradient
// or optimizer names enters the two tables above, so an inference or adjoint image still cannot name them.
#define SCOT_PLAN_TRAINING_ENTRY_POINTS(X)                                                                                          \
  SCOT_PLAN_ENTRY_POINTS(X)                                                                                                          \
  X(scot_loss_finish) X(scot_loss_bwd) X(scot_cln_bwd) X(scot_window_attn_bwd_rep) X(scot_block_tail_bwd) X(scot_proj_cln_bwd)      \
  X(scot_scale_inplace_dev) X(scot_pow2_rescale) X(scot_colscale_dev) X(scot_axpy_dev) X(scot_wgrad_group) X(scot_wgrad_mlp)        \
  X(scot_colsum) X(scot_conv5_wgrad) X(scot_dwconv7_wgrad) X(scot_nchw_channel_sum) X(scot_partial_colsum_batch)                    \
  X(scot_replica_reduce) X(scot_cpb_bwd_batched) X(scot_batch_sum) X(scot_segments_scale) X(scot_grad_sqnorm) X(scot_clip_coef)     \
  X(scot_adamw_step) X(scot_optim_finish) X(scot_transpose_cast)

// What every list of a two-stream image (formats 5 and 6) may call beside its own table: the engine's fork and join edges.
#define SCOT_PLAN_SYNC_ENTRY_POINTS(X) X(scot_event_record) X(scot_stream_wait_event)

// the three tables of entry points, and which of them each of the five call lists is held to; SYNC is admitted beside a list's own table
// in a two-stream image and nowhere else
enum { SCOT_PLAN_LIST_FORWARD, SCOT_PLAN_LIST_ADJOINT, SCOT_PLAN_LIST_TRAINING, SCOT_PLAN_LIST_SYNC, SCOT_PLAN_N_LISTS };
enum { SCOT_PLAN_SYNC_RECORD, SCOT_PLAN_SYNC_WAIT }; /* rows of SCOT_PLAN_LIST_SYNC */
enum { SCOT_PLAN_CALLS_FORWARD, SCOT_PLAN_CALLS_BACKWARD, SCOT_PLAN_CALLS_STEP_FORWARD, SCOT_PLAN_CALLS_STEP_BACKWARD,
       SCOT_PLAN_CALLS_UPDATE, SCOT_PLAN_N_CALLS };
#define SCOT_PLAN_NAME_STRING(n) #n,
static const char* const scot_plan_entry_names[] = {SCOT_PLAN_ENTRY_POINTS(SCOT_PLAN_NAME_STRING)};
static const char* const scot_plan_adjoint_entry_names[] = {SCOT_PLAN_ADJOINT_ENTRY_POINTS(SCOT_PLAN_NAME_STRING)};
static const char* const scot_plan_training_entry_names[] = {SCOT_PLAN_TRAINING_ENTRY_POINTS(SCOT_PLAN_NAME_STRING)};
static const char* const scot_plan_sync_entry_names[] = {SCOT_PLAN_SYNC_ENTRY_POINTS(SCOT_PLAN_NAME_STRING)};
#define SCOT_PLAN_COUNT(a) ((int)(sizeof(a) / sizeof((a)[0])))
static const struct {
  const char* const* names;
  int count;
} scot_plan_lists[SCOT_PLAN_N_LISTS] = {{scot_plan_entry_names, SCOT_PLAN_COUNT(scot_plan_entry_names)},
                                        {scot_plan_adjoint_entry_names, SCOT_PLAN_COUNT(scot_plan_adjoint_entry_names)},
                                        {scot_plan_training_entry_names, SCOT_PLAN_COUNT(scot_plan_training_entry_names)},
                                        {scot_plan_sync_entry_names, SCOT_PLAN_COUNT(scot_plan_sync_entry_names)}};

// the index of `name` in one of the three tables (SCOT_PLAN_LIST_*), -1: not listed there
static inline int scot_plan_list_index(const char* name, int list) {
  for (int i = 0; i < scot_plan_lists[list].count; ++i)
    if (strcmp(name, scot_plan_lists[list].names[i]) == 0) return i;
  return -1;
}

// status codes of the C ABI (common.h), restated so that this header needs nothing else
#define SCOT_PLAN_OK 0
#define SCOT_PLAN_ERR_SHAPE (-1)       /* malformed image: bounds, counts, relocations */
#define SCOT_PLAN_ERR_UNSUPPORTED (-3) /* well formed, but not for this library: ABI, operand format, format version, entry point */

typedef struct {
  const uint64_t* words; /* NULL, n = n_words = 0: the image has no such list */
  uint64_t n, n_words;   /* records, words */
  int names;             /* the table its names are held to (SCOT_PLAN_LIST_*) */
} scot_plan_calls;

typedef struct {
  const uint8_t* base;
  size_t bytes;
  const uint64_t* h;       /* header */
  const uint8_t* names;    /* n_names x SCOT_PLAN_NAME_BYTES */
  const uint64_t* buffers; /* n_buffers x 4 */
  const uint64_t* arrays;
  const uint64_t* io;
  const uint8_t* data;
  uint64_t format, n_names, n_buffers, n_arrays, arrays_words, data_bytes;
  scot_plan_calls calls[SCOT_PLAN_N_CALLS]; /* SCOT_PLAN_CALLS_* */
  const uint64_t* adj;   /* format 2 (NULL otherwise): the adjoint words */
  const uint64_t* train; /* formats 4 and 6 (NULL otherwise): the training words */
  uint64_t n_streams, n_events; /* 1 and 0 but in formats 5 and 6: what a STREAM and an EVENT pair may name */
} scot_plan_view;

// [off, off + n) inside [0, bytes), off 8-byte aligned, without overflow
static inline int scot_plan_span_ok(uint64_t off, uint64_t n, uint64_t bytes) {
  return (off & 7) == 0 && off <= bytes && n <= bytes - off;
}

// v->calls[slot] <- the list that the three words at `l` name (count, offset, words): inside the image, counts that cannot overflow
static inline int scot_plan_set_calls(scot_plan_view* v, int slot, int names, const uint64_t* l) {
  const uint64_t lim = (uint64_t)1 << 32;
  if (l[0] > lim || l[2] > lim || !scot_plan_span_ok(l[1], l[2] * 8, v->bytes)) return 0;
  v->calls[slot].words = (const uint64_t*)(v->base + l[1]);
  v->calls[slot].n = l[0];
  v->calls[slot].n_words = l[2];
  v->calls[slot].names = names;
  return 1;
}

// one argument pair: the tag is known, a relocation lies inside its buffer, an array index exists
static inline int scot_plan_arg_ok(const scot_plan_view* v, uint64_t tagw, uint64_t val, int in_array) {
  const uint64_t tag = tagw & 0xff, buf = tagw >> 8;
  switch (tag) {
    case SCOT_PLAN_ARG_INT:
    case SCOT_PLAN_ARG_NULL:
      return buf == 0;
    case SCOT_PLAN_ARG_STREAM:
      return buf == 0 && !in_array && val < v->n_streams;
    case SCOT_PLAN_ARG_EVENT:
      return buf == 0 && !in_array && val < v->n_events;
    case SCOT_PLAN_ARG_PTR:
      return buf < v->n_buffers && val < v->buffers[4 * buf + 1];      /* a pointer names a byte OF the buffer */
    case SCOT_PLAN_ARG_ARRAY:
      return buf == 0 && !in_array && val < v->n_arrays;
    default:
      return 0;
  }
}

// the words of the entry record at `e`: name, library, n_int, n_flt, the argument pairs, the floats
static inline uint64_t scot_plan_entry_words(const uint64_t* e) { return 4 + 2 * e[2] + e[3]; }

// the word offset of record `i` of a list (the list has been validated)
static inline uint64_t scot_plan_entry_at(const uint64_t* e, uint64_t i) {
  uint64_t w = 0;
  for (; i; --i) w += scot_plan_entry_words(e + w);
  return w;
}

// one call list: record bounds, n_int / n_flt, every argument pair, every name in the list's OWN table — or, in a two-stream image, in
// the SYNC table: a record is exactly (EVENT, STREAM), a wait exactly (STREAM, EVENT), and no other entry carries an EVENT pair.  The
// same pass holds the list to the closed-list rules of the header text; `recorded` (n_events bytes, the caller's) is scratch: the stream
// + 1 of an event's latest record in THIS list.
static inline int scot_plan_entries_ok(const scot_plan_view* v, const scot_plan_calls* c, uint8_t* recorded) {
  const uint64_t* e = c->words;
  uint64_t w = 0;
  /* side: 0 = stream 1 not used yet, 1 = open (entries on stream 1 that stream 0 has not waited for), 2 = joined; join_event: the event
     of the record that is the last entry on stream 1 so far (n_events: that entry is no record) */
  int side = 0;
  uint64_t join_event = v->n_events;
  memset(recorded, 0, (size_t)v->n_events);
  for (uint64_t i = 0; i < c->n; ++i, w += scot_plan_entry_words(e + w)) {
    if (c->n_words - w < 4) return SCOT_PLAN_ERR_SHAPE;
    const uint64_t name = e[w], lib = e[w + 1], ni = e[w + 2], nf = e[w + 3];
    if (name >= v->n_names || lib > 1 || ni > SCOT_PLAN_MAX_INT || nf > SCOT_PLAN_MAX_FLT) return SCOT_PLAN_ERR_SHAPE;
    if (scot_plan_entry_words(e + w) > c->n_words - w) return SCOT_PLAN_ERR_SHAPE;
    uint64_t on = 0, events = 0;      /* the stream this entry is issued on, the EVENT pairs it carries */
    for (uint64_t k = 0; k < ni; ++k) {
      if (!scot_plan_arg_ok(v, e[w + 4 + 2 * k], e[w + 5 + 2 * k], 0)) return SCOT_PLAN_ERR_SHAPE;
      if ((e[w + 4 + 2 * k] & 0xff) == SCOT_PLAN_ARG_STREAM) on |= e[w + 5 + 2 * k];
      events += (e[w + 4 + 2 * k] & 0xff) == SCOT_PLAN_ARG_EVENT;
    }
    for (uint64_t k = 0; k < nf; ++k)
      if (e[w + 4 + 2 * ni + k] >> 32) return SCOT_PLAN_ERR_SHAPE;      /* raw bits of ONE float */
    const char* nm = (const char*)(v->names + name * SCOT_PLAN_NAME_BYTES);
    const int sync = v->n_streams > 1 ? scot_plan_list_index(nm, SCOT_PLAN_LIST_SYNC) : -1;
    if (sync < 0 && scot_plan_list_index(nm, c->names) < 0) return SCOT_PLAN_ERR_UNSUPPORTED;
    if (sync < 0 && events) return SCOT_PLAN_ERR_SHAPE;
    uint64_t ev = v->n_events;
    if (sync >= 0) {
      const int at = sync == SCOT_PLAN_SYNC_RECORD ? 0 : 1;      /* where the EVENT pair sits; the STREAM pair is the other one */
      if (ni != 2 || nf != 0 || (e[w + 4 + 2 * at] & 0xff) != SCOT_PLAN_ARG_EVENT || (e[w + 6 - 2 * at] & 0xff) != SCOT_PLAN_ARG_STREAM)
        return SCOT_PLAN_ERR_SHAPE;
      ev = e[w + 5 + 2 * at];
      if (sync == SCOT_PLAN_SYNC_WAIT && !recorded[ev]) return SCOT_PLAN_ERR_SHAPE;      /* no earlier record in this list */
    }
    if (on) {
      /* the first entry on stream 1: a wait for a record on stream 0 of this list */
      if (!side && !(sync == SCOT_PLAN_SYNC_WAIT && recorded[ev] == 1)) return SCOT_PLAN_ERR_SHAPE;
      side = 1;
      join_event = sync == SCOT_PLAN_SYNC_RECORD ? ev : v->n_events;
    } else if (sync == SCOT_PLAN_SYNC_WAIT && ev == join_event && recorded[ev] == 2) {
      side = 2;      /* stream 0 is behind everything stream 1 has been given so far */
    }
    if (sync == SCOT_PLAN_SYNC_RECORD) recorded[ev] = (uint8_t)(on + 1);
  }
  if (side == 1) return SCOT_PLAN_ERR_SHAPE;      /* the list leaves stream 1 unjoined */
  return w == c->n_words ? SCOT_PLAN_OK : SCOT_PLAN_ERR_SHAPE;
}

// THE span rule of the io, adjoint and training words: `n` bytes at `off` of buffer `buf` lie whole inside a buffer of kind `kind`
static inline int scot_plan_io_span_ok(const scot_plan_view* v, uint64_t buf, uint64_t off, uint64_t n, uint64_t kind) {
  if (buf >= v->n_buffers || n == 0) return 0;
  const uint64_t cap = v->buffers[4 * buf + 1];
  return off <= cap && n <= cap - off && v->buffers[4 * buf] == kind;
}

// the spans (buffer, offset, bytes) at words[slot..slot + 2]: each holds exactly the expected bytes, and, unless that is 0 (an absent
// span), obeys the span rule for its kind
typedef struct {
  uint64_t slot, bytes, kind;
} scot_plan_want;

static inline int scot_plan_spans_ok(const scot_plan_view* v, const uint64_t* words, const scot_plan_want* want, int n) {
  for (int s = 0; s < n; ++s) {
    const uint64_t* sp = words + want[s].slot;
    if (sp[2] != want[s].bytes) return 0;
    if (sp[2] && !scot_plan_io_span_ok(v, sp[0], sp[1], sp[2], want[s].kind)) return 0;
  }
  return 1;
}

// array `index` of the arrays section -> its kind and count (the section has been validated)
static inline void scot_plan_array_at(const scot_plan_view* v, uint64_t index, uint64_t* kind, uint64_t* count) {
  uint64_t w = 0;
  for (uint64_t i = 0; i < index; ++i) w += 2 + 2 * v->arrays[w + 1];
  *kind = v->arrays[w];
  *count = v->arrays[w + 1];
}

// the training words of a format-4 image, after everything else has been validated: the lr patch point names an array of exactly
// `groups` floats of an update entry called scot_adamw_step; labels in an input buffer, loss and prediction in output buffers, every
// state span whole inside a STATE buffer that the image initialises (so none can touch a constant)
static inline int scot_plan_training_ok(const scot_plan_view* v) {
  const uint64_t* t = v->train;
  const uint64_t* io = v->io;
  const scot_plan_calls* upd = &v->calls[SCOT_PLAN_CALLS_UPDATE];
  const uint64_t groups = t[SCOT_PLAN_TR_GROUPS], floats = t[SCOT_PLAN_TR_ARENA_FLOATS];
  const uint64_t flags = t[SCOT_PLAN_TR_FLAGS];
  if (flags > 7 || groups < 1 || groups > 8 || floats == 0 || floats % 8 || floats > ((uint64_t)1 << 36)) return SCOT_PLAN_ERR_SHAPE;
  /* the batch's pixel_mask: the io words hold a mask input exactly when FLAGS says the batch has one, of the bytes its kind needs */
  if (((flags & SCOT_PLAN_TR_FLAG_MASK) != 0) != (io[SCOT_PLAN_IO_HAS_MASK] != 0)) return SCOT_PLAN_ERR_SHAPE;
  if ((flags & SCOT_PLAN_TR_FLAG_MASK_FULL) && !(flags & SCOT_PLAN_TR_FLAG_MASK)) return SCOT_PLAN_ERR_SHAPE;
  if ((flags & SCOT_PLAN_TR_FLAG_MASK) &&
      io[SCOT_PLAN_IO_MASK_BYTES] != io[SCOT_PLAN_IO_B] * io[SCOT_PLAN_IO_COUT] *
                                         ((flags & SCOT_PLAN_TR_FLAG_MASK_FULL) ? io[SCOT_PLAN_IO_H] * io[SCOT_PLAN_IO_W] : 1))
    return SCOT_PLAN_ERR_SHAPE;
  for (int c = SCOT_PLAN_CALLS_STEP_FORWARD; c <= SCOT_PLAN_CALLS_UPDATE; ++c)
    if (!v->calls[c].n) return SCOT_PLAN_ERR_SHAPE;
  if (t[SCOT_PLAN_TR_LR_ENTRY] >= upd->n) return SCOT_PLAN_ERR_SHAPE;
  const uint64_t* e = upd->words + scot_plan_entry_at(upd->words, t[SCOT_PLAN_TR_LR_ENTRY]);
  if (strcmp((const char*)(v->names + e[0] * SCOT_PLAN_NAME_BYTES), "scot_adamw_step") != 0) return SCOT_PLAN_ERR_SHAPE;
  /* (the weight-decay array behind it has the same kind and length: only lr's own position is a patch point) */
  if (t[SCOT_PLAN_TR_LR_ARG] != SCOT_PLAN_ADAMW_LR_ARG || t[SCOT_PLAN_TR_LR_ARG] >= e[2] ||
      (e[4 + 2 * t[SCOT_PLAN_TR_LR_ARG]] & 0xff) != SCOT_PLAN_ARG_ARRAY)
    return SCOT_PLAN_ERR_SHAPE;
  uint64_t kind = 0, count = 0;
  scot_plan_array_at(v, e[5 + 2 * t[SCOT_PLAN_TR_LR_ARG]], &kind, &count);
  if (kind != 2 || count != groups) return SCOT_PLAN_ERR_SHAPE;
  const uint64_t out_bytes = io[SCOT_PLAN_IO_B] * io[SCOT_PLAN_IO_COUT] * io[SCOT_PLAN_IO_H] * io[SCOT_PLAN_IO_W] * 4;
  const uint64_t dyn = t[SCOT_PLAN_TR_FLAGS] & 1, half = t[SCOT_PLAN_TR_SHADOW + 2] ? floats * 2 : 0;
  const scot_plan_want want[12] = {{SCOT_PLAN_TR_LABELS, out_bytes, SCOT_PLAN_BUF_INPUT},
                                   {SCOT_PLAN_TR_LOSS, 4, SCOT_PLAN_BUF_OUTPUT},
                                   {SCOT_PLAN_TR_PRED, out_bytes, SCOT_PLAN_BUF_OUTPUT},
                                   {SCOT_PLAN_TR_ARENA, floats * 4, SCOT_PLAN_BUF_STATE},
                                   {SCOT_PLAN_TR_EXP_AVG, floats * 4, SCOT_PLAN_BUF_STATE},
                                   {SCOT_PLAN_TR_EXP_AVG_SQ, floats * 4, SCOT_PLAN_BUF_STATE},
                                   {SCOT_PLAN_TR_SHADOW, half, SCOT_PLAN_BUF_STATE},
                                   {SCOT_PLAN_TR_SHADOW_T, (uint64_t)(t[SCOT_PLAN_TR_SHADOW_T + 2] ? half : 0), SCOT_PLAN_BUF_STATE},
                                   {SCOT_PLAN_TR_STEP_STATE, 8, SCOT_PLAN_BUF_STATE},
                                   {SCOT_PLAN_TR_CLIP, 12, SCOT_PLAN_BUF_STATE},
                                   {SCOT_PLAN_TR_SCALE_STATE, (uint64_t)(dyn ? 16 : 0), SCOT_PLAN_BUF_STATE},
                                   {SCOT_PLAN_TR_COUNTER, (uint64_t)(dyn ? 4 : 0), SCOT_PLAN_BUF_STATE}};
  if (!scot_plan_spans_ok(v, t, want, 12)) return SCOT_PLAN_ERR_SHAPE;
  if (t[SCOT_PLAN_TR_SHADOW_T + 2] && !t[SCOT_PLAN_TR_SHADOW + 2]) return SCOT_PLAN_ERR_SHAPE;
  for (int a = 0; a < 12; ++a) {
    const uint64_t* x = t + want[a].slot;
    if (!x[2]) continue;
    /* a STATE span is stored by value */
    if (want[a].kind == SCOT_PLAN_BUF_STATE && v->buffers[4 * x[0] + 3] != 1) return SCOT_PLAN_ERR_SHAPE;
    /* no two spans share a byte: labels, loss, prediction and every piece of state are distinct memory */
    for (int b = a + 1; b < 12; ++b) {
      const uint64_t* y = t + want[b].slot;
      if (y[2] && x[0] == y[0] && x[1] < y[1] + y[2] && y[1] < x[1] + x[2]) return SCOT_PLAN_ERR_SHAPE;
    }
  }
  return SCOT_PLAN_OK;
}

// Validates the whole image before anything is allocated: section bounds, counts, every relocation inside its buffer, every name in
// the table of its list, and a format version, ABI and operand format equal to the caller's (the library's own).  Fills *v with pointers
// INTO the image.  `image` must be 8-byte aligned.
static inline int scot_plan_image_validate(const void* image, size_t bytes, int abi, int operand_format, scot_plan_view* v) {
  memset(v, 0, sizeof(*v));
  if (!image || ((uintptr_t)image & 7) || bytes < SCOT_PLAN_HEADER_WORDS * 8) return SCOT_PLAN_ERR_SHAPE;
  const uint8_t* b = (const uint8_t*)image;
  const uint64_t* h = (const uint64_t*)image;
  if (h[SCOT_PLAN_H_MAGIC] != SCOT_PLAN_MAGIC) return SCOT_PLAN_ERR_SHAPE;
  const uint64_t format = h[SCOT_PLAN_H_FORMAT];
  if (format != SCOT_PLAN_FORMAT && format != SCOT_PLAN_FORMAT_ADJOINT && format != SCOT_PLAN_FORMAT_TRAINING &&
      format != SCOT_PLAN_FORMAT_STREAMS && format != SCOT_PLAN_FORMAT_TRAINING_STREAMS)
    return SCOT_PLAN_ERR_UNSUPPORTED;
  const int streamed = format == SCOT_PLAN_FORMAT_STREAMS || format == SCOT_PLAN_FORMAT_TRAINING_STREAMS;
  const int adjoint = format == SCOT_PLAN_FORMAT_ADJOINT;
  const int training = format == SCOT_PLAN_FORMAT_TRAINING || format == SCOT_PLAN_FORMAT_TRAINING_STREAMS;
  const int enabled[SCOT_PLAN_N_LISTS] = {1, adjoint, training, streamed};      /* the tables of entry points this format may name */
  if (h[SCOT_PLAN_H_ABI] != (uint64_t)abi || h[SCOT_PLAN_H_OPERAND] != (uint64_t)operand_format) return SCOT_PLAN_ERR_UNSUPPORTED;
  if (h[SCOT_PLAN_H_BYTES] != (uint64_t)bytes) return SCOT_PLAN_ERR_SHAPE;      /* a truncated (or padded) file */
  v->base = b;
  v->bytes = bytes;
  v->h = h;
  v->format = h[SCOT_PLAN_H_FORMAT];
  v->n_names = h[SCOT_PLAN_H_NNAMES];
  v->n_buffers = h[SCOT_PLAN_H_NBUFFERS];
  v->n_arrays = h[SCOT_PLAN_H_NARRAYS];
  v->arrays_words = h[SCOT_PLAN_H_ARRAYS_WORDS];
  v->data_bytes = h[SCOT_PLAN_H_DATA_BYTES];
  v->n_streams = 1;
  if (streamed) {      // the streams section: exactly two streams, a bounded number of events
    if (!scot_plan_span_ok(h[SCOT_PLAN_H_STREAMS_OFF], SCOT_PLAN_STREAMS_WORDS * 8, bytes)) return SCOT_PLAN_ERR_SHAPE;
    const uint64_t* st = (const uint64_t*)(b + h[SCOT_PLAN_H_STREAMS_OFF]);
    if (st[SCOT_PLAN_ST_STREAMS] != 2 || st[SCOT_PLAN_ST_EVENTS] > SCOT_PLAN_MAX_EVENTS) return SCOT_PLAN_ERR_SHAPE;
    v->n_streams = st[SCOT_PLAN_ST_STREAMS];
    v->n_events = st[SCOT_PLAN_ST_EVENTS];
  }
  const uint64_t lim = (uint64_t)1 << 32;      /* counts that cannot overflow the products below */
  if (v->n_names > lim || v->n_buffers > lim || v->n_arrays > lim || v->arrays_words > lim) return SCOT_PLAN_ERR_SHAPE;
  if (!scot_plan_span_ok(h[SCOT_PLAN_H_NAMES_OFF], v->n_names * SCOT_PLAN_NAME_BYTES, bytes) ||
      !scot_plan_span_ok(h[SCOT_PLAN_H_BUFFERS_OFF], v->n_buffers * 32, bytes) ||
      !scot_plan_span_ok(h[SCOT_PLAN_H_ARRAYS_OFF], v->arrays_words * 8, bytes) ||
      !scot_plan_span_ok(h[SCOT_PLAN_H_IO_OFF], SCOT_PLAN_IO_WORDS * 8, bytes) ||
      !scot_plan_span_ok(h[SCOT_PLAN_H_DATA_OFF], v->data_bytes, bytes))
    return SCOT_PLAN_ERR_SHAPE;
  // the call lists: the forward and (format 2) the backward are named by header words ...
  if (!scot_plan_set_calls(v, SCOT_PLAN_CALLS_FORWARD, SCOT_PLAN_LIST_FORWARD, h + SCOT_PLAN_H_NENTRIES)) return SCOT_PLAN_ERR_SHAPE;
  if (adjoint) {
    if (!scot_plan_set_calls(v, SCOT_PLAN_CALLS_BACKWARD, SCOT_PLAN_LIST_ADJOINT, h + SCOT_PLAN_H_NBACKWARD) ||
        !scot_plan_span_ok(h[SCOT_PLAN_H_ADJ_OFF], SCOT_PLAN_ADJ_WORDS * 8, bytes))
      return SCOT_PLAN_ERR_SHAPE;
    v->adj = (const uint64_t*)(b + h[SCOT_PLAN_H_ADJ_OFF]);
  }
  if (training) {      // ... the three step lists (format 4) by training words
    if (!scot_plan_span_ok(h[SCOT_PLAN_H_TRAIN_OFF], SCOT_PLAN_TRAIN_WORDS * 8, bytes)) return SCOT_PLAN_ERR_SHAPE;
    v->train = (const uint64_t*)(b + h[SCOT_PLAN_H_TRAIN_OFF]);
    for (int s = 0; s < 3; ++s)
      if (!scot_plan_set_calls(v, SCOT_PLAN_CALLS_STEP_FORWARD + s, SCOT_PLAN_LIST_TRAINING, v->train + SCOT_PLAN_TR_FWD + 3 * s))
        return SCOT_PLAN_ERR_SHAPE;
  }
  v->names = b + h[SCOT_PLAN_H_NAMES_OFF];
  v->buffers = (const uint64_t*)(b + h[SCOT_PLAN_H_BUFFERS_OFF]);
  v->arrays = (const uint64_t*)(b + h[SCOT_PLAN_H_ARRAYS_OFF]);
  v->io = (const uint64_t*)(b + h[SCOT_PLAN_H_IO_OFF]);
  v->data = b + h[SCOT_PLAN_H_DATA_OFF];
  // names: terminated, and listed in a table this format allows (each entry is then held to its own list's)
  for (uint64_t i = 0; i < v->n_names; ++i) {
    const char* nm = (const char*)(v->names + i * SCOT_PLAN_NAME_BYTES);
    if (!memchr(nm, 0, SCOT_PLAN_NAME_BYTES)) return SCOT_PLAN_ERR_SHAPE;
    int listed = 0;
    for (int l = 0; l < SCOT_PLAN_N_LISTS; ++l) listed |= enabled[l] && scot_plan_list_index(nm, l) >= 0;
    if (!listed) return SCOT_PLAN_ERR_UNSUPPORTED;
  }
  // buffers: a known kind, a size, a constant's content inside the data section
  for (uint64_t i = 0; i < v->n_buffers; ++i) {
    const uint64_t kind = v->buffers[4 * i], n = v->buffers[4 * i + 1], off = v->buffers[4 * i + 2];
    if (kind > (uint64_t)(adjoint || training ? SCOT_PLAN_BUF_STATE : SCOT_PLAN_BUF_SCRATCH) || n == 0 || n > ((uint64_t)1 << 40)) return SCOT_PLAN_ERR_SHAPE;
    if (kind == SCOT_PLAN_BUF_CONSTANT && !scot_plan_span_ok(off, n, v->data_bytes)) return SCOT_PLAN_ERR_SHAPE;
    if (training && kind == SCOT_PLAN_BUF_STATE) {      // stored by value (1) or zeroed at load (0)
      const uint64_t init = v->buffers[4 * i + 3];
      if (init > 1 || (init && !scot_plan_span_ok(off, n, v->data_bytes))) return SCOT_PLAN_ERR_SHAPE;
    }
  }
  // arrays
  uint64_t w = 0;
  for (uint64_t i = 0; i < v->n_arrays; ++i) {
    if (v->arrays_words - w < 2) return SCOT_PLAN_ERR_SHAPE;
    const uint64_t kind = v->arrays[w], cnt = v->arrays[w + 1];
    if (kind > (uint64_t)(training ? 2 : 1) || cnt > (v->arrays_words - w - 2) / 2) return SCOT_PLAN_ERR_SHAPE;
    for (uint64_t k = 0; k < cnt; ++k) {
      const uint64_t tagw = v->arrays[w + 2 + 2 * k], val = v->arrays[w + 3 + 2 * k];
      if (!scot_plan_arg_ok(v, tagw, val, 1)) return SCOT_PLAN_ERR_SHAPE;
      if (kind != 1 && (tagw & 0xff) != SCOT_PLAN_ARG_INT) return SCOT_PLAN_ERR_SHAPE;
      if (kind == 2 && (val >> 32)) return SCOT_PLAN_ERR_SHAPE;      /* raw bits of ONE float */
      if (kind == 1 && (tagw & 0xff) == SCOT_PLAN_ARG_INT) return SCOT_PLAN_ERR_SHAPE;
    }
    w += 2 + 2 * cnt;
  }
  if (w != v->arrays_words) return SCOT_PLAN_ERR_SHAPE;
  // every call list against its own table, by the same rules (an absent list has no records and no words)
  uint8_t recorded[SCOT_PLAN_MAX_EVENTS];
  for (int c = 0; c < SCOT_PLAN_N_CALLS; ++c) {
    const int erc = scot_plan_entries_ok(v, &v->calls[c], recorded);
    if (erc != SCOT_PLAN_OK) return erc;
  }
  // io: fp32 [B, Cin, H, W] in, fp32 [B, Cout, H, W] out, each whole inside a buffer of the right kind
  const uint64_t* io = v->io;
  const uint64_t B = io[SCOT_PLAN_IO_B], Cin = io[SCOT_PLAN_IO_CIN], H = io[SCOT_PLAN_IO_H], W = io[SCOT_PLAN_IO_W], Cout = io[SCOT_PLAN_IO_COUT];
  if (!B || !Cin || !H || !W || !Cout || B > 65536 || Cin > 65536 || Cout > 65536 || H > 65536 || W > 65536) return SCOT_PLAN_ERR_SHAPE;
  if (B * Cin * H * W > ((uint64_t)1 << 38) || B * Cout * H * W > ((uint64_t)1 << 38)) return SCOT_PLAN_ERR_SHAPE;
  const uint64_t in_bytes = B * Cin * H * W * 4, out_bytes = B * Cout * H * W * 4;
  const uint64_t spans[4][4] = {      /* present (0 / 1), slot of the (buffer, offset) pair, bytes, kind */
      {1, SCOT_PLAN_IO_PV_BUF, in_bytes, SCOT_PLAN_BUF_INPUT},
      {io[SCOT_PLAN_IO_HAS_TIME], SCOT_PLAN_IO_TIME_BUF, io[SCOT_PLAN_IO_TIME_BYTES], SCOT_PLAN_BUF_INPUT},
      {io[SCOT_PLAN_IO_HAS_MASK], SCOT_PLAN_IO_MASK_BUF, io[SCOT_PLAN_IO_MASK_BYTES], SCOT_PLAN_BUF_INPUT},
      {1, SCOT_PLAN_IO_OUT_BUF, out_bytes, SCOT_PLAN_BUF_OUTPUT}};
  for (int s = 0; s < 4; ++s) {
    if (spans[s][0] > 1) return SCOT_PLAN_ERR_SHAPE;
    if (spans[s][0] && !scot_plan_io_span_ok(v, io[spans[s][1]], io[spans[s][1] + 1], spans[s][2], spans[s][3])) return SCOT_PLAN_ERR_SHAPE;
  }
  if (io[SCOT_PLAN_IO_HAS_TIME] && io[SCOT_PLAN_IO_TIME_BYTES] != B * 4) return SCOT_PLAN_ERR_SHAPE;
  if (adjoint) {
    // the cotangent's copy is an input, the gradients are outputs, the scale and its counter are the runtime's own
    const uint64_t* a = v->adj;
    const uint64_t flags = a[SCOT_PLAN_ADJ_FLAGS], scaled = a[SCOT_PLAN_ADJ_STATE + 2];
    if (flags > 3 || (flags && !v->calls[SCOT_PLAN_CALLS_BACKWARD].n)) return SCOT_PLAN_ERR_SHAPE;
    if ((flags & 2) && !io[SCOT_PLAN_IO_HAS_TIME]) return SCOT_PLAN_ERR_SHAPE;
    const scot_plan_want want[5] = {{SCOT_PLAN_ADJ_COT, out_bytes, SCOT_PLAN_BUF_INPUT},
                                    {SCOT_PLAN_ADJ_DPV, (flags & 1) ? in_bytes : 0, SCOT_PLAN_BUF_OUTPUT},
                                    {SCOT_PLAN_ADJ_DTIME, (flags & 2) ? B * 4 : 0, SCOT_PLAN_BUF_OUTPUT},
                                    {SCOT_PLAN_ADJ_STATE, (uint64_t)(scaled ? 16 : 0), SCOT_PLAN_BUF_STATE},
                                    {SCOT_PLAN_ADJ_COUNTER, (uint64_t)(scaled ? 4 : 0), SCOT_PLAN_BUF_STATE}};
    if (!scot_plan_spans_ok(v, a, want, 5)) return SCOT_PLAN_ERR_SHAPE;
    const int64_t e = (int64_t)a[SCOT_PLAN_ADJ_SCALE_EXP];
    if (e < -120 || e > 120 || (e != 0 && !scaled)) return SCOT_PLAN_ERR_SHAPE;
  }
  if (training) return scot_plan_training_ok(v);
  return SCOT_PLAN_OK;
}
#endif
