/* fcsjg.h — joint genotyping of one-sample GVCF records on the GPU
 * (libfcship.so, gfx950).
 *
 * The rules are DESIGN §2 [EXT] "GenotypeGVCFs, round 20" (§4.13): a sample's
 * source record at a site, the exact allele-frequency model per ALT in int64
 * fixed point (2^-20 of a PL), the site decision, and every sample's GT, GQ
 * and PLs over REF and the kept ALTs.  Reading GVCFs, building the site table
 * and formatting records is host code (host/gvcf.h, host/joint.h).  Everything
 * that crosses the device boundary is an integer.  Errors follow fcship.h: a
 * negative FCS_ERR_* code and a "[E::fcsjg_...] ..." message from
 * fcs_last_error().
 */
#ifndef FCSJG_H
#define FCSJG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCSJG_SAMPLES_MAX 1024   /* larger cohorts are refused (int64 holds 4,096 rows of clamped PLs) */
#define FCSJG_ALTS_MAX 6         /* ALTs per site */
#define FCSJG_PL_MAX 1048575     /* 2^20 - 1; larger PLs are clamped by the reader */
#define FCSJG_UNIT_BITS 20       /* a log value's unit is 2^-20 of a PL */
#define FCSJG_S_ROWS 1282        /* the log-sum table */
#define FCSJG_GENOTYPES_MAX 28   /* genotypes of REF and six ALTs */
#define FCSJG_KIND_BLOCK 0       /* ALT <NON_REF>, three PLs */
#define FCSJG_KIND_CALL 1        /* ALT X,<NON_REF>, six PLs */
#define FCSJG_NO_CALL 255        /* gt of a sample without a call */

/* the _dev entry point's status word */
#define FCSJG_STATUS_FIELD 1     /* a PL outside 0 .. FCSJG_PL_MAX or a record range outside n_records, clamped */
#define FCSJG_STATUS_PL 2        /* more PLs than max_pl: none beyond it written */

/* One contig of the cohort: sample s's records are rec_off[s] .. rec_off[s + 1],
 * in file order. */
typedef struct {
  int32_t n_samples;       /* 1 .. FCSJG_SAMPLES_MAX */
  int32_t reserved;
  int64_t n_records;
  const int64_t* rec_off;  /* [n_samples + 1] non-decreasing, rec_off[n_samples] <= n_records */
  const int32_t* beg;      /* [n_records] 0-based POS; non-decreasing within a sample */
  const int32_t* end;      /* [n_records] one past the last position: END for a block, beg + len(REF) for a call */
  const uint8_t* kind;     /* [n_records] FCSJG_KIND_* */
  const uint8_t* alt;      /* [n_records] a call's ALT as the merged index 1 .. n_alt of the site at beg; 0: cut */
  const int32_t* dp;       /* [n_records] */
  const int32_t* pl;       /* [n_records][6] VCF genotype order; a block's last three are not read */
} fcsjg_cohort;

typedef struct {
  int64_t n_sites;
  const int32_t* pos;      /* [n_sites] 0-based, ascending */
  const uint8_t* n_alt;    /* [n_sites] 1 .. FCSJG_ALTS_MAX */
} fcsjg_sites;

/* fcsjg_tables' three tables for the cohort's n_samples, and the threshold. */
typedef struct {
  const int32_t* S;        /* [FCSJG_S_ROWS] */
  const int32_t* LG;       /* [4 n_samples + 1] */
  const int32_t* LP;       /* [2 n_samples + 1] */
  int64_t min_qual;        /* a site is written when QUAL >= min_qual (units) */
} fcsjg_model;

typedef struct {
  int64_t* q;              /* [n_sites][6] per ALT; an ALT the site lacks: 0 */
  int32_t* mle;            /* [n_sites][6] */
  int64_t* qual;           /* [n_sites] sum of q over the kept ALTs */
  uint8_t* kept;           /* [n_sites] bit i - 1: ALT i has mle > 0 */
  int32_t* ac;             /* [n_sites][6] per ALT, from the GTs; zero at a site that is not written */
  int32_t* an;             /* [n_sites] */
  int64_t* dp;             /* [n_sites] sum of DP over the samples with a source */
  int64_t* pl_off;         /* [n_sites] the site's first PL, -1 when the site is not written */
  int64_t* src;            /* [n_sites][n_samples] the source record, -1 without one */
  uint8_t* gt;             /* [n_sites][n_samples][2] merged alleles, FCSJG_NO_CALL without a call or at a site not written */
  uint8_t* gq;             /* [n_sites][n_samples] */
  int32_t* pl;             /* [max_pl] the written sites' PLs: [sample][genotype of REF and the kept ALTs] */
  int64_t max_pl;
  int64_t* n_pl;           /* PLs of all written sites, also when above max_pl */
} fcsjg_out;

/* S[i] = llround(10 log10(1 + 10^(-i / 160)) 2^20), LG[n] = llround(10 log10(n)
 * 2^20) (LG[0] = 0), LP[k] from heterozygosity h: h / k for k >= 1 and
 * 1 - sum(h / k, k = 1 .. 2 n_samples) for k = 0.  Host only: no device is
 * touched.  Refused: n_samples outside 1 .. FCSJG_SAMPLES_MAX, h outside (0, 1),
 * a prior of k = 0 that is not positive. */
int fcsjg_tables(double heterozygosity, int32_t n_samples, int32_t* S, int32_t* LG, int32_t* LP);

/* Host pointers.  Every field is checked before the device is touched; then
 * one H2D copy, the kernels on a leased session's stream, the outputs copied
 * back.  The outputs are written only on FCS_OK.  Refused: offsets out of
 * order, a sample's positions that decrease, beg >= end, a kind, ALT index or
 * PL out of range, positions of sites that do not ascend, n_alt outside
 * 1 .. 6, more PLs than max_pl. */
int fcsjg_genotype(int32_t device, const fcsjg_cohort* cohort, const fcsjg_sites* sites, const fcsjg_model* model,
                   const fcsjg_out* out);

/* Bytes of device workspace fcsjg_genotype_dev needs (negative: FCS_ERR_INVALID). */
int64_t fcsjg_workspace_bytes(int64_t n_sites, int32_t n_samples);

/* Device pointers inside *cohort, *sites, *model and *out (the structs
 * themselves are in host memory); all work is queued on `stream`, without
 * synchronisation.  Only the scalar arguments are checked; the kernels clamp
 * every PL and record range and OR what they met into *dev_status
 * (FCSJG_STATUS_*), which the caller zeroes. */
int fcsjg_genotype_dev(int32_t device, const fcsjg_cohort* cohort, const fcsjg_sites* sites, const fcsjg_model* model,
                       const fcsjg_out* out, void* dev_workspace, int64_t workspace_bytes, int32_t* dev_status,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FCSJG_H */
