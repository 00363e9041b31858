/* fcsug.h — pileup SNP genotyping on the GPU (libfcship.so, gfx950).
 *
 * The rules are DESIGN §2 [EXT] "UnifiedGenotyper, SNP model" (§4.12): which
 * records and which of their bases are counted at a reference position, the
 * integer sums a locus keeps, and which loci are sites.  fcsug_sites piles a
 * batch up over one window of one contig and returns the window's sites,
 * ascending by offset; genotyping a site is host code (host/ug.h).  Everything
 * that crosses the device boundary is an integer.  Errors follow fcship.h: a
 * negative FCS_ERR_* code and a "[E::fcsug_...] ..." message from
 * fcs_last_error().
 */
#ifndef FCSUG_H
#define FCSUG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCSUG_TILE 256            /* loci per tile */
#define FCSUG_WINDOW_MAX 16777216 /* loci per window */
#define FCSUG_TABLE_ROWS 94       /* effective qualities 0 .. 93 */

/* the _dev entry point's status word */
#define FCSUG_STATUS_FIELD 1      /* an offset or CIGAR outside the declared sizes, clamped; the record adds nothing */
#define FCSUG_STATUS_REF 2        /* an aligned base beyond its contig, not counted */
#define FCSUG_STATUS_ORDER 4      /* positions decrease: no site is produced */
#define FCSUG_STATUS_SITES 8      /* more sites than max_sites: none beyond it written */

/* fcsdp_batch's fields; bases (ASCII, one byte per read base, at the offsets of qual) ARE read. */
typedef struct {
  int64_t n;                 /* records */
  const uint16_t* flag;      /* [n] BAM flags */
  const int32_t* ref_id;     /* [n] */
  const int32_t* pos;        /* [n] 0-based leftmost; non-decreasing among the records of the window's contig */
  const uint8_t* mapq;       /* [n] */
  const uint32_t* cigar;     /* BAM CIGAR words; record r's are cigar_off[r] .. cigar_off[r + 1] */
  const int64_t* cigar_off;  /* [n + 1] non-decreasing, cigar_off[n] <= n_cigar */
  int64_t n_cigar;
  const uint8_t* bases;      /* ASCII letters; record r's are base_off[r] .. base_off[r + 1] */
  const uint8_t* qual;       /* phred bytes, at the same offsets */
  const int64_t* base_off;   /* [n + 1] */
  int64_t n_bases;
  const uint8_t* qual_absent; /* [n] non-zero: the record has no qualities (q = 0 for every base) */
} fcsug_batch;

typedef struct {
  int32_t min_baseq;  /* counted bases: min(q, MAPQ, 93) >= min_baseq */
} fcsug_params;

/* Loci [start, start + len) of contig ref_id, which has contig_len bases. */
typedef struct {
  int32_t ref_id;
  int32_t reserved;
  int64_t start, len, contig_len;
} fcsug_window;

/* One site.  ref and alt are letter codes (A C G T = 0 .. 3); n, qsum per
 * letter code; gl in units of 2^-32 log10 for ref/ref, ref/alt, alt/alt. */
typedef struct {
  int32_t offset;  /* window offset */
  uint8_t ref, alt;
  uint16_t reserved;
  uint32_t n[4], qsum[4], n_del, reserved2;
  uint64_t mq2;
  int64_t gl[3];
} fcsug_site; /* 80 bytes */

/* T[q][c] = llround(log10(p_c) * 2^32) for q = 0 .. 93 and c = 0, 1, 2 (DESIGN
 * §2).  Host only: no device is touched.  0 < pcr_error < 1. */
int fcsug_table(double pcr_error, int64_t* table /* [94][3] */);

/* Host pointers.  Every field is checked before the device is touched; then
 * one H2D copy, the kernels on a leased session's stream, the sites copied
 * back.  sites[0, *n_sites) and *n_sites are written only on FCS_OK.  Refused:
 * offsets out of order, a counted record whose CIGAR does not cover its bases
 * or with an aligned base beyond contig_len, positions that decrease among the
 * records of the window's contig, more sites than max_sites. */
int fcsug_sites(int32_t device, const fcsug_batch* batch, const fcsug_params* params, const fcsug_window* window,
                const uint8_t* ref /* [len] ASCII */, const int64_t* table, fcsug_site* sites, int64_t max_sites,
                int64_t* n_sites);

/* Bytes of device workspace fcsug_sites_dev needs (negative: FCS_ERR_INVALID). */
int64_t fcsug_workspace_bytes(int64_t n_records, int64_t len);

/* Device pointers inside *batch (the struct itself is in host memory) and in
 * every other pointer argument; all work is queued on `stream`, without
 * synchronisation.  Only the scalar arguments are checked; the kernels clamp
 * every offset to the declared sizes and OR what they met into *dev_status
 * (FCSUG_STATUS_*), which the caller zeroes.  *dev_n_sites is the number of
 * sites found, also when it is above max_sites. */
int fcsug_sites_dev(int32_t device, const fcsug_batch* batch, const fcsug_params* params, const fcsug_window* window,
                    const uint8_t* dev_ref, const int64_t* dev_table, fcsug_site* dev_sites, int64_t max_sites,
                    int64_t* dev_n_sites, void* dev_workspace, int64_t workspace_bytes, int32_t* dev_status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FCSUG_H */
