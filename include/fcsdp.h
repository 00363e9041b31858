/* fcsdp.h — depth of coverage on the GPU (libfcship.so, gfx950).
 *
 * The rules are DESIGN §2 [EXT] "Depth of coverage" (§4.11): which records and
 * which of their bases add 1 to the depth of a reference position, and the
 * 501-bin histogram, totals and granular quantiles of the loci that take part.
 * fcsdp_count adds a batch's depths over one window of one contig;
 * fcsdp_stats summarises pieces of a window.  Errors follow fcship.h: a
 * negative FCS_ERR_* code and a "[E::fcsdp_...] ..." message from
 * fcs_last_error().
 */
#ifndef FCSDP_H
#define FCSDP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCSDP_BINS 501             /* bin d for depth d = 0 .. 499, bin 500 for depth >= 500 */
#define FCSDP_PIECE_MAX 65536      /* loci per piece at most */
#define FCSDP_WINDOW_MAX 1073741824LL /* loci per window at most (2^30) */
#define FCSDP_ABOVE 15             /* the "%_bases_above_15" threshold: depth >= 15 */

/* the _dev entry points' status word */
#define FCSDP_STATUS_FIELD 1    /* an offset, CIGAR or piece outside the declared sizes, clamped */
#define FCSDP_STATUS_REF 2      /* an aligned base beyond its contig, not counted */
#define FCSDP_STATUS_OVERFLOW 4 /* a depth beyond the signed 32-bit cells */

/* fcsbq_batch's fields without rg.  bases is never read (the base letter does
 * not matter) and may be null. */
typedef struct {
  int64_t n;                 /* records */
  const uint16_t* flag;      /* [n] BAM flags */
  const int32_t* ref_id;     /* [n] */
  const int32_t* pos;        /* [n] 0-based leftmost */
  const uint8_t* mapq;       /* [n] */
  const uint32_t* cigar;     /* BAM CIGAR words; record r's are cigar_off[r] .. cigar_off[r + 1] */
  const int64_t* cigar_off;  /* [n + 1] non-decreasing, cigar_off[n] <= n_cigar */
  int64_t n_cigar;
  const uint8_t* bases;      /* unused */
  const uint8_t* qual;       /* phred bytes; record r's are base_off[r] .. base_off[r + 1] */
  const int64_t* base_off;   /* [n + 1] */
  int64_t n_bases;
  const uint8_t* qual_absent; /* [n] non-zero: the record has no qualities (q = 0 for every base) */
} fcsdp_batch;

typedef struct {
  int32_t min_mapq, max_mapq;   /* counted records: min_mapq <= MAPQ <= max_mapq */
  int32_t min_baseq, max_baseq; /* counted bases: min_baseq <= q <= max_baseq */
  int32_t include_deletions;    /* non-zero: every deleted position adds 1 */
} fcsdp_params;

/* Loci [start, start + len) of contig ref_id, which has contig_len bases. */
typedef struct {
  int32_t ref_id;
  int32_t reserved;
  int64_t start, len, contig_len;
} fcsdp_window;

/* Loci [start, end) of a window, end - start <= FCSDP_PIECE_MAX.  long_index
 * is -1 for an interval that is this one piece, else the interval's row of
 * long_hist. */
typedef struct {
  int32_t start, end, long_index, reserved;
} fcsdp_piece;

/* Over a piece's participating loci.  The quantiles are the reported ones
 * (max(bin, 1); 1 without loci); they are 0 for a piece with a long_index. */
typedef struct {
  uint64_t total;
  uint32_t loci, above;
  uint32_t q1, median, q3, reserved;
} fcsdp_summary;

/* Host pointers.  Every field is checked before the device is touched; then
 * one H2D copy, the kernels on a leased session's stream, one D2H copy.  The
 * batch's depths over the window are ADDED to depth[len], only on FCS_OK.  A
 * counted record with an aligned base beyond contig_len is refused. */
int fcsdp_count(int32_t device, const fcsdp_batch* batch, const fcsdp_params* params, const fcsdp_window* window,
                uint32_t* depth);

/* bitmap: bit i & 63 of word i >> 6 is set when window locus i takes part
 * ((len + 63) / 64 words).  Adds to hist[501] and long_hist[n_long][501] and
 * writes summary[n_pieces], only on FCS_OK. */
int fcsdp_stats(int32_t device, const uint32_t* depth, const uint64_t* bitmap, int64_t len, const fcsdp_piece* pieces,
                int64_t n_pieces, int32_t n_long, uint64_t* hist, uint64_t* long_hist, fcsdp_summary* summary);

/* Bytes of device workspace fcsdp_scan_dev needs for a window of len loci (negative: FCS_ERR_INVALID). */
int64_t fcsdp_workspace_bytes(int64_t len);

/* Device pointers inside *batch (the struct itself is in host memory) and in
 * every other pointer argument; all work is queued on `stream`, without
 * synchronisation.  Only the scalar arguments are checked; the kernels clamp
 * every offset to the declared sizes and OR what they met into *dev_status
 * (FCSDP_STATUS_*), which the caller zeroes.  A record with a clamped field
 * adds nothing.
 *
 * fcsdp_runs_dev adds the batch's run ends (+1 at a run's first window offset,
 * -1 one past its last) to dev_cells[len + 1]; several batches may accumulate.
 * fcsdp_scan_dev turns dev_cells[0, len) into depths in place.
 * fcsdp_stats_dev reads the depths as uint32_t; a piece with a clamped field is
 * summarised over its clamped range and adds to no long_hist row. */
int fcsdp_runs_dev(int32_t device, const fcsdp_batch* batch, const fcsdp_params* params, const fcsdp_window* window,
                   int32_t* dev_cells, int32_t* dev_status, void* stream);
int fcsdp_scan_dev(int32_t device, int32_t* dev_cells, int64_t len, void* dev_workspace, int64_t workspace_bytes,
                   int32_t* dev_status, void* stream);
int fcsdp_stats_dev(int32_t device, const uint32_t* dev_depth, const uint64_t* dev_bitmap, int64_t len,
                    const fcsdp_piece* dev_pieces, int64_t n_pieces, int32_t n_long, uint64_t* dev_hist,
                    uint64_t* dev_long_hist, fcsdp_summary* dev_summary, int32_t* dev_status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FCSDP_H */
