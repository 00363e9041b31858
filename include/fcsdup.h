/* fcsdup.h — duplicate marking on the GPU (libfcship.so, gfx950).
 *
 * The rules are Picard MarkDuplicates' criteria as sambamba restates them
 * (DESIGN §2 [EXT], §4.9).  A batch is every primary, secondary and
 * supplementary record of one read-group job or of one BAM, as
 * structure-of-arrays; the call answers dup[r] = 1 for the records that are
 * to carry 0x400.  Errors follow fcship.h: a negative FCS_ERR_* code and a
 * "[E::fcsdup_mark] ..." message from fcs_last_error().
 *
 * Key widths: at most FCSDUP_MAX_REFS reference sequences, FCSDUP_MAX_LIBS
 * libraries, |unclipped 5' position| < FCSDUP_MAX_POS, at most
 * FCSDUP_MAX_QUAL quality bytes per record and FCSDUP_MAX_RECORDS records.
 * A batch beyond them is refused (FCS_ERR_INVALID): keys never collide.
 */
#ifndef FCSDUP_H
#define FCSDUP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCSDUP_MAX_REFS 2097151   /* 2^21 - 1 */
#define FCSDUP_MAX_LIBS 2047      /* 2^11 - 1 */
#define FCSDUP_MAX_POS 1073741824 /* 2^30 */
#define FCSDUP_MAX_QUAL 4194304   /* 2^22 */
#define FCSDUP_MAX_RECORDS 1073741824

/* fcsdup_mark_dev's status word */
#define FCSDUP_STATUS_POS 1    /* an unclipped 5' position beyond FCSDUP_MAX_POS */
#define FCSDUP_STATUS_FIELD 2  /* a ref_id, lib or offset outside the batch's declared ranges */

typedef struct {
  int64_t n;                /* records */
  const uint16_t* flag;     /* [n] BAM flags */
  const int32_t* ref_id;    /* [n] in [-1, n_ref) */
  const int32_t* pos;       /* [n] 0-based leftmost */
  const int32_t* mate;      /* [n] index of the primary record of the template's other read (primary records only), or -1;
                               symmetric: mate[mate[r]] == r */
  const int32_t* lib;       /* [n] in [0, n_lib) */
  const uint32_t* cigar;    /* BAM CIGAR words (len << 4 | op); record r's are cigar_off[r] .. cigar_off[r + 1] */
  const int64_t* cigar_off; /* [n + 1] non-decreasing, cigar_off[n] <= n_cigar */
  int64_t n_cigar;
  const uint8_t* qual;      /* phred bytes; record r's are qual_off[r] .. qual_off[r + 1] (none: quality absent) */
  const int64_t* qual_off;  /* [n + 1] */
  int64_t n_qual;
  int32_t n_ref, n_lib;
} fcsdup_batch;

typedef struct {
  int64_t examined;   /* records that are none of unmapped, secondary, supplementary */
  int64_t pairs;      /* pairs of two examined mates */
  int64_t fragments;  /* examined records that are not paired */
  int64_t duplicates; /* records flagged */
} fcsdup_stats;

/* Host pointers.  Every offset, mate, ref_id and lib is checked before any
 * device work; then one H2D copy, the kernels on a leased session's stream,
 * one D2H copy.  dup[n] and *stats are written only on FCS_OK. */
int fcsdup_mark(int32_t device, const fcsdup_batch* batch, uint8_t* dup, fcsdup_stats* stats);

/* Bytes of device workspace fcsdup_mark_dev needs for n records (negative: FCS_ERR_INVALID). */
int64_t fcsdup_workspace_bytes(int64_t n);

/* Device pointers inside *batch (the struct itself is in host memory), all
 * work queued on `stream`, no synchronisation.  Only the scalar arguments
 * are checked; the kernels clamp every offset and index to the declared
 * sizes and report what they clamped in *dev_status (FCSDUP_STATUS_*, 0 when
 * the result is valid).  qual must lie in an allocation that starts and ends
 * on a 4-byte boundary (every hipMalloc does): it is read as aligned dwords. */
int fcsdup_mark_dev(int32_t device, const fcsdup_batch* batch, void* dev_workspace, int64_t workspace_bytes,
                    uint8_t* dev_dup, fcsdup_stats* dev_stats, int32_t* dev_status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FCSDUP_H */
