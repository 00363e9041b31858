/* fcsir.h — indel realignment's scoring step on the GPU (libfcship.so, gfx950).
 *
 * The rules are DESIGN §2 [EXT] "RealignerTargetCreator and IndelRealigner,
 * round 22" (§4.14).  A bin is one realignment target with its candidate
 * consensus sequences and its alt reads.  fcsir_score answers, for every
 * (consensus, alt read) pair of every bin of a batch, the smallest score S of
 * the read against the consensus over the candidate offsets (the read's
 * original offset and every offset at which the read fits) and the offset that
 * has it: among equals the original offset, then the smallest.  Everything else
 * of the command is host code (host/indel.h).  Everything that crosses the
 * device boundary is an integer.  Errors follow fcship.h: a negative FCS_ERR_*
 * code and a "[E::fcsir_...] ..." message from fcs_last_error().
 */
#ifndef FCSIR_H
#define FCSIR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCSIR_READ_MAX 512        /* bases of a read */
#define FCSIR_SEQ_MAX 4096        /* bases of a sequence */
#define FCSIR_OVERHANG 99         /* S per read base beyond the sequence's end */
#define FCSIR_ORIG_MAX 1073741824 /* the largest original offset */

/* the _dev entry point's status word */
#define FCSIR_STATUS_FIELD 1 /* an offset, a length or an original offset outside the declared sizes, clamped */
#define FCSIR_STATUS_PAIRS 2 /* more pairs than max_pairs: none beyond it written */

/* Codes are 0 .. 3 for A C G T and 4 for anything else.  Bin b has the
 * sequences bin_seq[b] .. bin_seq[b + 1] and the reads bin_read[b] ..
 * bin_read[b + 1]; with C_b and R_b of them, its pairs begin at pair_first[b] =
 * sum of C_a R_a over a < b, and the pair of its consensus c and read r is
 * pair_first[b] + c R_b + r. */
typedef struct {
  int64_t n_bins, n_seq, n_reads;
  int64_t n_seq_bytes, n_read_bytes;
  const uint8_t* seq;       /* codes; sequence s's are seq_off[s] .. seq_off[s + 1], 1 .. FCSIR_SEQ_MAX of them */
  const int64_t* seq_off;   /* [n_seq + 1] non-decreasing, seq_off[n_seq] <= n_seq_bytes */
  const int64_t* bin_seq;   /* [n_bins + 1] from 0 to n_seq */
  const uint8_t* read;      /* codes; read r's are read_off[r] .. read_off[r + 1], 1 .. FCSIR_READ_MAX of them */
  const uint8_t* qual;      /* phred bytes, at the same offsets */
  const int64_t* read_off;  /* [n_reads + 1] */
  const int64_t* bin_read;  /* [n_bins + 1] from 0 to n_reads */
  const int32_t* orig;      /* [n_reads] the read's original offset in its bin's sequences, 0 .. FCSIR_ORIG_MAX */
} fcsir_batch;

/* Host pointers.  Every field is checked before the device is touched; then
 * one H2D copy, the kernels on a leased session's stream, one copy back.
 * best[0, *n_pairs), off[0, *n_pairs) and *n_pairs are written only on FCS_OK.
 * Refused: offsets out of order or beyond the sizes, an empty or too long
 * sequence or read, a code above 4, an original offset outside its range, more
 * pairs than max_pairs. */
int fcsir_score(int32_t device, const fcsir_batch* batch, uint32_t* best, int32_t* off, int64_t max_pairs, int64_t* n_pairs);

/* Bytes of device workspace fcsir_score_dev needs (negative: FCS_ERR_INVALID). */
int64_t fcsir_workspace_bytes(int64_t n_bins);

/* Device pointers inside *batch (the struct itself is in host memory) and in
 * every other pointer argument; all work is queued on `stream`, without
 * synchronisation.  Only the scalar arguments are checked; the kernels clamp
 * every offset and length to the declared sizes and OR what they met into
 * *dev_status (FCSIR_STATUS_*), which the caller zeroes.  *dev_n_pairs is the
 * number of pairs, also when it is above max_pairs. */
int fcsir_score_dev(int32_t device, const fcsir_batch* batch, uint32_t* dev_best, int32_t* dev_off, int64_t max_pairs,
                    int64_t* dev_n_pairs, void* dev_workspace, int64_t workspace_bytes, int32_t* dev_status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FCSIR_H */
