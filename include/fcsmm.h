/* fcsmm.h — the chaining recurrence of minimizer seeding on the GPU
 * (libfcship.so, gfx950).
 *
 * The rules are DESIGN §2 [EXT] "minimizer seeding and chaining" (§4.16).  A
 * read's anchors are (t, q) pairs sorted by (t, q): t = (contig * 2 + rev) << 32
 * | position of the k-mer's last base on the forward reference, q the position
 * of its last base in the oriented read.  fcsmm_chain answers, for every anchor
 * i of every read of a batch, the chaining score f[i] and the predecessor p[i]
 * (an index within the read, or -1) over the candidates j in [i - FCSMM_LOOKBACK,
 * i - 1].  Sketching, the index, the backtrack and everything after it are host
 * code (host/minimizer.h).  Everything that crosses the device boundary is an
 * integer.  Errors follow fcship.h: a negative FCS_ERR_* code and a
 * "[E::fcsmm_...] ..." message from fcs_last_error().
 */
#ifndef FCSMM_H
#define FCSMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCSMM_LOOKBACK 64           /* candidate predecessors of an anchor */
#define FCSMM_SPAN_MAX 64           /* the largest span */
#define FCSMM_GAP_MAX 1048576       /* the largest max_gap and bw */
#define FCSMM_READ_ANCHORS 16777216 /* the most anchors of one read */

/* the _dev entry point's status word */
#define FCSMM_STATUS_FIELD 1 /* a read's offsets outside the declared sizes or out of order: the read skipped */
#define FCSMM_STATUS_ORDER 2 /* a read's anchors are not sorted by (t, q) */

/* Read r has the anchors read_off[r] .. read_off[r + 1]. */
typedef struct {
  int64_t n_reads, n_anchors;
  const int64_t* t;        /* [n_anchors] target keys, >= 0 */
  const int32_t* q;        /* [n_anchors] query positions, >= 0 */
  const int64_t* read_off; /* [n_reads + 1] non-decreasing, read_off[n_reads] <= n_anchors */
  int32_t max_gap, bw;     /* 0 .. FCSMM_GAP_MAX */
  int32_t span;            /* 1 .. FCSMM_SPAN_MAX */
  int32_t reserved;        /* zero */
} fcsmm_batch;

/* Host pointers.  Every field is checked before the device is touched; then
 * one H2D copy, the kernel on a leased session's stream, one copy back.  f and
 * p ([n_anchors] each; the entries of anchors no read holds are left alone) are
 * written only on FCS_OK.  Refused: offsets out of order or beyond the sizes, a
 * read with more than FCSMM_READ_ANCHORS anchors, a negative t or q, anchors of a
 * read not sorted by (t, q), a parameter outside its range. */
int fcsmm_chain(int32_t device, const fcsmm_batch* batch, int32_t* f, int32_t* p);

/* Bytes of device workspace fcsmm_chain_dev needs (negative: FCS_ERR_INVALID). */
int64_t fcsmm_workspace_bytes(int64_t n_reads, int64_t n_anchors);

/* Device pointers inside *batch (the struct itself is in host memory) and in
 * every other pointer argument; all work is queued on `stream`, without
 * synchronisation.  Only the scalar arguments are checked; the kernel reads and
 * writes nothing outside the declared sizes: a read whose two offsets are out
 * of order, beyond n_anchors or more than FCSMM_READ_ANCHORS apart is skipped,
 * and what the kernel met is ORed into *dev_status (FCSMM_STATUS_*), which the
 * caller zeroes.  A read with unsorted anchors still gets an f and a p.  A read
 * whose offsets and order are sound gets the same f and p whatever the other
 * reads hold. */
int fcsmm_chain_dev(int32_t device, const fcsmm_batch* batch, int32_t* dev_f, int32_t* dev_p, void* dev_workspace,
                    int64_t workspace_bytes, int32_t* dev_status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FCSMM_H */
