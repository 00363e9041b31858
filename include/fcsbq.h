/* fcsbq.h — base quality recalibration on the GPU (libfcship.so, gfx950).
 *
 * The rules are GATK 4's BaseRecalibrator and ApplyBQSR at their defaults as
 * DESIGN §2 [EXT] restates them (§4.10): mismatch events, the covariates read
 * group, quality, context (2 bases) and cycle.  fcsbq_count adds a batch's
 * observations and errors to the context and cycle tables; the host finalises
 * them (host/bqsr.h) into three tables of doubles; fcsbq_apply rewrites the
 * batch's qualities from those.  Errors follow fcship.h: a negative FCS_ERR_*
 * code and a "[E::fcsbq_...] ..." message from fcs_last_error().
 */
#ifndef FCSBQ_H
#define FCSBQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCSBQ_NQ 94          /* qualities 0 .. 93 */
#define FCSBQ_NCTX 16        /* context keys 4 * prev + cur */
#define FCSBQ_NCYC 1000      /* cycle keys 2 * (|c| - 1) + (c < 0), |c| <= FCSBQ_MAX_CYCLE */
#define FCSBQ_MAX_CYCLE 500  /* counted (kept) or applied bases per record */
#define FCSBQ_MAX_RG 1024
#define FCSBQ_MAX_BASES 4294967295LL /* bases per call: below 2^32 */

/* the _dev entry points' status word */
#define FCSBQ_STATUS_FIELD 1 /* an offset, ref_id, rg or CIGAR outside the declared sizes, clamped */
#define FCSBQ_STATUS_REF 2   /* an aligned base beyond its contig, not counted */
#define FCSBQ_STATUS_LONG 4  /* a record of more than FCSBQ_MAX_CYCLE bases */

typedef struct {
  int64_t n;                 /* records */
  const uint16_t* flag;      /* [n] BAM flags */
  const int32_t* ref_id;     /* [n] */
  const int32_t* pos;        /* [n] 0-based leftmost */
  const uint8_t* mapq;       /* [n] */
  const int32_t* rg;         /* [n] in [-1, n_rg) */
  const uint32_t* cigar;     /* BAM CIGAR words; record r's are cigar_off[r] .. cigar_off[r + 1] */
  const int64_t* cigar_off;  /* [n + 1] non-decreasing, cigar_off[n] <= n_cigar */
  int64_t n_cigar;
  const uint8_t* bases;      /* one ASCII byte per base; record r's are base_off[r] .. base_off[r + 1] */
  const uint8_t* qual;       /* phred bytes at the same offsets */
  const int64_t* base_off;   /* [n + 1] */
  int64_t n_bases;
  const uint8_t* qual_absent; /* [n] non-zero: the record has no qualities (its qual bytes are ignored) */
} fcsbq_batch;

typedef struct fcsbq_ref fcsbq_ref;

/* A device copy of the reference: the contigs' bytes (either case) one after
 * the other, ref_off[n_ref + 1] their starts, and the known-sites bitmap, bit
 * g & 63 of word g >> 6 for the concatenated position g ((ref_off[n_ref] + 63)
 * / 64 words). */
int fcsbq_ref_create(int32_t device, const uint8_t* bases, const int64_t* ref_off, int32_t n_ref,
                     const uint64_t* known_bits, fcsbq_ref** handle);
int fcsbq_ref_destroy(fcsbq_ref* handle);

/* Host pointers.  Every field is checked before the device is touched; then
 * one H2D copy, the kernels on a leased session's stream, one D2H copy.  The
 * batch's counts are ADDED to ctx[n_rg][94][16][2] and cyc[n_rg][94][1000][2]
 * ((observations, errors) pairs), only on FCS_OK. */
int fcsbq_count(const fcsbq_ref* handle, const fcsbq_batch* batch, int32_t n_rg, int64_t* ctx, int64_t* cyc);

/* base[n_rg][94], dctx[n_rg][94][16], dcyc[n_rg][94][1000]; out_qual: n_bases
 * bytes in the batch's layout (records that are not recalibrated are copied),
 * written only on FCS_OK. */
int fcsbq_apply(int32_t device, const fcsbq_batch* batch, int32_t n_rg, const double* base, const double* dctx,
                const double* dcyc, uint8_t* out_qual);

/* Bytes of device workspace fcsbq_count_dev needs for n_rg read groups (negative: FCS_ERR_INVALID). */
int64_t fcsbq_workspace_bytes(int32_t n_rg);

/* Device pointers inside *batch (the struct itself is in host memory) and in
 * every other pointer argument; all work is queued on `stream`, without
 * synchronisation.  Only the scalar arguments are checked; the kernels clamp
 * every offset and index to the declared sizes and report what they clamped in
 * *dev_status (FCSBQ_STATUS_*).  When the status is not 0, nothing is added to
 * the tables and nothing is written to dev_out_qual. */
int fcsbq_count_dev(const fcsbq_ref* handle, const fcsbq_batch* batch, int32_t n_rg, void* dev_workspace,
                    int64_t workspace_bytes, int64_t* dev_ctx, int64_t* dev_cyc, int32_t* dev_status, void* stream);
int fcsbq_apply_dev(int32_t device, const fcsbq_batch* batch, int32_t n_rg, const double* dev_base,
                    const double* dev_dctx, const double* dev_dcyc, uint8_t* dev_out_qual, int32_t* dev_status,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FCSBQ_H */
