/* fcspu.h — the pileup in front of htc's and mutect2's PairHMM on the GPU
 * (libfcship.so, gfx950).
 *
 * The rules are csrc/pu_rules.h: which aligned bases count at a
 * locus, what they add to its depth, its events and its three reference-model
 * sums, which loci are active sites and which single-base alleles at least two
 * reads carry.  fcspu_pile piles one or two batches up over one window of one
 * contig.  The sums in double are added read after read in the order of the
 * batch, so they equal the host's bit for bit.  Errors follow fcship.h: a
 * negative FCS_ERR_* code and a "[E::fcspu_...] ..." message from
 * fcs_last_error().
 */
#ifndef FCSPU_H
#define FCSPU_H

#include <stdint.h>

#include "fcsug.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FCSPU_TILE 256            /* loci per block; a wave owns 64 consecutive loci */
#define FCSPU_WINDOW_MAX 16777216 /* loci per window */
#define FCSPU_TABLE_ROWS 94       /* qualities 0 .. 93 */
#define FCSPU_BATCHES_MAX 2

/* the _dev entry point's status word */
#define FCSPU_STATUS_FIELD 1      /* an offset or CIGAR outside the declared sizes, clamped; the record adds nothing */
#define FCSPU_STATUS_REF 2        /* an aligned base beyond its contig, not counted */
#define FCSPU_STATUS_ORDER 4      /* positions decrease: nothing is piled up, no array is written, both counts are 0 */
#define FCSPU_STATUS_SITES 8      /* more sites than max_sites: none beyond it written */
#define FCSPU_STATUS_SNVS 16      /* more SNVs than max_snvs: none beyond it written */
#define FCSPU_STATUS_LETTER 32    /* a counted read letter other than A C G T N: the base is not counted */

/* A batch is an fcsug_batch: bases are ASCII.  Of its records those of the
 * window's contig are piled up, every one of them: flag, mapq and qual_absent
 * are not read (the caller has filtered its records, as htc's decoder does).
 * In mutect2 batch 0 is the tumor and batch 1 the normal. */
typedef fcsug_batch fcspu_batch;
typedef fcsug_window fcspu_window;

typedef struct {
  int32_t min_bq;   /* counted bases: quality >= min_bq */
  int32_t want_gl;  /* non-zero: gl is written */
  double frac;      /* a site: events >= 2 and events >= frac * max(1, depth) */
} fcspu_params;

/* A single-base allele that at least two reads (of all batches) carry. */
typedef struct {
  int32_t offset;  /* window offset */
  uint8_t alt;     /* the read letter, A C G or T */
  uint8_t reserved[3];
  int32_t count;
} fcspu_snv; /* 12 bytes */

/* Where the results go.  depth and events are sums over all batches; events
 * holds the mismatch events of aligned bases only: the events of insertions
 * and deletions are counted per CIGAR op by the caller, which adds them
 * afterwards.  gl (want_gl) is batch 0's alone, 3 doubles per locus.  sites
 * are the offsets where batch 0's depth and its events, the mismatch events
 * plus events_in's, meet the predicate, ascending.  snvs ascend by (offset, alt). */
typedef struct {
  int32_t* depth;   /* [len] */
  int32_t* events;  /* [len] */
  double* gl;       /* [3 * len], or null without want_gl */
  int32_t* sites;   /* [max_sites] */
  int64_t max_sites;
  int64_t* n_sites;
  fcspu_snv* snvs;  /* [max_snvs] */
  int64_t max_snvs;
  int64_t* n_snvs;
} fcspu_out;

/* T[q][0] = log10(1 - e), T[q][1] = log10(0.5 (1 - e) + 0.5 e / 3), T[q][2] =
 * log10(e / 3) with e = min(0.75, 10^(-q / 10)), for q = 0 .. 93.  Host only,
 * and the one entry of this header that libfcsgenome.so exports, not
 * libfcship.so: the table is filled by the caller's own reference model
 * (host/pileup.h), so that the device adds the very doubles the host adds. */
int fcspu_table(double* table /* [94][3] */);

/* Host pointers.  Every field is checked before the device is touched; then
 * one H2D copy, the kernels on a leased session's stream, the results copied
 * back.  events_in (nullable, [len]): batch 0's events of insertions and
 * deletions, which the site predicate adds to batch 0's mismatch events.
 * Nothing is written unless the call returns FCS_OK.  Refused: offsets out of
 * order, a record of the window's contig whose CIGAR does not cover its bases
 * or with an aligned base beyond contig_len, positions that decrease among the
 * records of the window's contig, a counted read letter other than A C G T N
 * (the message names the record), more sites than max_sites, more SNVs than
 * max_snvs (the message names both numbers). */
int fcspu_pile(int32_t device, const fcspu_batch* batches, int32_t n_batches, const fcspu_params* params,
               const fcspu_window* window, const uint8_t* ref /* [len] ASCII */, const double* table,
               const int32_t* events_in, const fcspu_out* out);

/* Bytes of device workspace fcspu_pile_dev needs for batches of n_records[0 ..
 * n_batches) records (negative: FCS_ERR_INVALID). */
int64_t fcspu_workspace_bytes(const int64_t* n_records, int32_t n_batches, int64_t len);

/* Device pointers inside the batches and *out (the structs themselves are in
 * host memory) and in every other pointer argument; all work is queued on
 * `stream`, without synchronisation.  Only the scalar arguments are checked;
 * the kernels clamp every offset to the declared sizes and OR what they met
 * into *dev_status (FCSPU_STATUS_*), which the caller zeroes.  *out->n_sites
 * and *out->n_snvs are the numbers found, also when they are above the maxima. */
int fcspu_pile_dev(int32_t device, const fcspu_batch* batches, int32_t n_batches, const fcspu_params* params,
                   const fcspu_window* window, const uint8_t* dev_ref, const double* dev_table,
                   const int32_t* dev_events_in, const fcspu_out* out, void* dev_workspace, int64_t workspace_bytes,
                   int32_t* dev_status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FCSPU_H */
