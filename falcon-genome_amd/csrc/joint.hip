// Joint genotyping on the device (include/fcsjg.h; DESIGN §2 [EXT], §4.13).
// The rules are csrc/jg_model.h (one text for these kernels, host/joint.cpp and
// tools/micro/jg_test.cpp).  All work of a call is queued on one stream,
// without a host round trip.  The (site, sample) matrices are site-major.
//
// jg_source_kernel: a lane per (site, sample): two binary searches over the
// sample's records give the source record, or -1 for a no-call.
// jg_source_kernel is built for 8 waves per SIMD.
//
// jg_model_kernel<NP>: a wave per (site, ALT).  Allele count k = 64 p + lane is
// pass p of a lane, NP passes in registers (2 n_samples + 1 <= 64 NP).  Samples
// are taken 64 at a time, a lane collapsing one sample's PLs to c0, c1, c2; the
// called ones are rows, their three g values read from the owning lane and so
// wave-uniform.  Row j runs only the passes with 64 p <= 2j; z[k - 1] and
// z[k - 2] arrive by a lane rotation of the row before, lanes 0 and 1 taking
// them from the rotation of the pass below (the carry between a lane's passes).
// S and the live part of LG (4 n_samples + 1 entries) sit in LDS.  The sum over
// k for q runs in ascending k on values read lane by lane; mle is a wave arg-max
// with ties to the smaller k.
// jg_model_kernel<1> is built for 8 waves per SIMD.
// jg_model_kernel<2> is built for 8 waves per SIMD.
// jg_model_kernel<3> is built for 8 waves per SIMD.
// jg_model_kernel<5> is built for 7 waves per SIMD.
// jg_model_kernel<9> is built for 5 waves per SIMD.
// jg_model_kernel<17> is built for 4 waves per SIMD.
// jg_model_kernel<33> is built for 2 waves per SIMD.
//
// jg_site_kernel: a lane per site: the kept mask, QUAL, the decision and the
// site's number of PLs; AC, AN and DP zeroed.
// jg_site_kernel is built for 8 waves per SIMD.
//
// jg_scan_kernel: the exclusive scan of the sites' PL counts by one block, in
// passes of 256 sites; the total and the "more PLs than max_pl" bit.
// jg_scan_kernel is built for 8 waves per SIMD.
//
// jg_geno_kernel: a lane per (site, sample) of the written sites: the PLs over
// REF and the kept ALTs at the site's offset, GT, GQ, and the site's AC, AN and
// DP by integer atomics.
// jg_geno_kernel is built for 8 waves per SIMD.
//
// Every loop is bounded by a count of sites, samples, records or alleles; no
// kernel uses scratch.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "fcship_internal.h"
#include "fcsjg.h"
#include "jg_model.h"
#include "rec_batch.h"

namespace fcs {

namespace {

constexpr int kJgBlock = 256;
constexpr int kJgWaves = kJgBlock / 64;
// launch caps of the stride loops
constexpr int kJgCellMaxBlocks = 1024;   // jg_source_kernel, jg_geno_kernel: a lane per (site, sample)
constexpr int kJgModelMaxBlocks = 2048;  // jg_model_kernel: a wave per (site, ALT)
constexpr int kJgSiteMaxBlocks = 64;     // jg_site_kernel: a lane per site

static_assert(FCSJG_ALTS_MAX == kJgAltsMax && FCSJG_PL_MAX == kJgPlMax && FCSJG_S_ROWS == kJgSRows &&
                  FCSJG_UNIT_BITS == kJgUnitBits && FCSJG_GENOTYPES_MAX == kJgGenotypesMax,
              "fcsjg.h and jg_model.h");
static_assert(FCSJG_KIND_BLOCK == kJgKindBlock && FCSJG_KIND_CALL == kJgKindCall && FCSJG_NO_CALL == kJgNoCall &&
                  FCSJG_STATUS_FIELD == kJgStatusField && FCSJG_STATUS_PL == kJgStatusPl,
              "fcsjg.h and jg_model.h");
static_assert(2 * FCSJG_SAMPLES_MAX + 1 <= 64 * 33, "the widest jg_model_kernel holds the largest cohort");
static_assert(sizeof(fcsjg_cohort) == 72 && sizeof(fcsjg_sites) == 24 && sizeof(fcsjg_model) == 32 && sizeof(fcsjg_out) == 112,
              "argument layouts");

__global__ __launch_bounds__(kJgBlock) void jg_source_kernel(fcsjg_cohort c, fcsjg_sites st, int64_t* __restrict__ src,
                                                             int32_t* __restrict__ status) {
  const int64_t cells = st.n_sites * c.n_samples;
  for (int64_t i = (int64_t)blockIdx.x * kJgBlock + threadIdx.x; i < cells; i += (int64_t)gridDim.x * kJgBlock) {
    const int64_t site = i / c.n_samples;
    const int s = (int)(i - site * c.n_samples);
    const int64_t o0 = c.rec_off[s], o1 = c.rec_off[s + 1];
    const int64_t lo = clamp64(o0, 0, c.n_records), hi = clamp64(o1, lo, c.n_records);
    if (lo != o0 || hi != o1) atomicOr(status, kJgStatusField);
    src[i] = jg_source(c.beg, c.end, c.kind, lo, hi, st.pos[site]);
  }
}

__device__ __forceinline__ int64_t jg_rotate(int64_t v, int lane, int by) { return __shfl(v, (lane - by) & 63); }

template <int NP>
__global__ __launch_bounds__(kJgBlock) void jg_model_kernel(fcsjg_cohort c, fcsjg_sites st, fcsjg_model m,
                                                            const int64_t* __restrict__ src, int64_t* __restrict__ q,
                                                            int32_t* __restrict__ mle) {
  __shared__ int32_t S[kJgSRows];
  __shared__ int32_t LG[128 * NP];
  const int tid = (int)threadIdx.x, wave = tid / 64, lane = tid % 64;
  const int n_samples = c.n_samples;  // 2 n_samples + 1 <= 64 NP: the launcher's choice of NP
  for (int k = tid; k < kJgSRows; k += kJgBlock) S[k] = m.S[k];
  for (int k = tid; k < 128 * NP; k += kJgBlock) LG[k] = k <= 4 * n_samples ? m.LG[k] : 0;
  __syncthreads();
  const int64_t items = st.n_sites * kJgAltsMax;
  for (int64_t it = (int64_t)blockIdx.x * kJgWaves + wave; it < items; it += (int64_t)gridDim.x * kJgWaves) {
    const int64_t site = it / kJgAltsMax;
    const int i = (int)(it - site * kJgAltsMax) + 1;
    const int n_alt = st.n_alt[site] < kJgAltsMax ? st.n_alt[site] : kJgAltsMax;
    if (i > n_alt) {
      if (lane == 0) q[it] = 0, mle[it] = 0;
      continue;
    }
    int64_t z[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) z[p] = 0;  // z_0[0] = 1
    int j = 0;
    for (int s0 = 0; s0 < n_samples; s0 += 64) {
      int32_t cc[3] = {0, 0, 0};
      bool called = false;
      if (s0 + lane < n_samples) {
        const int64_t r = src[site * n_samples + s0 + lane];
        if (r >= 0) {
          const int kind = c.kind[r];
          jg_collapse(kind, c.alt[r], n_alt, i, jg_load_pl(c.pl + 6 * r, kind), cc);
          called = true;
        }
      }
      uint64_t rows = __ballot(called);
      while (rows) {
        const int t = __ffsll((unsigned long long)rows) - 1;
        rows &= rows - 1;
        ++j;
        const int64_t g0 = -((int64_t)__shfl(cc[0], t) << kJgUnitBits), g1 = -((int64_t)__shfl(cc[1], t) << kJgUnitBits),
                      g2 = -((int64_t)__shfl(cc[2], t) << kJgUnitBits);
        int64_t below1 = 0, below2 = 0;  // the rotations of the pass below, row j - 1
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          if (64 * p > 2 * j) continue;  // wave-uniform
          const int64_t r1 = jg_rotate(z[p], lane, 1), r2 = jg_rotate(z[p], lane, 2);
          const int64_t z1 = lane >= 1 ? r1 : below1, z2 = lane >= 2 ? r2 : below2;
          below1 = r1, below2 = r2;
          const int k = 64 * p + lane;
          if (k <= 2 * j) z[p] = jg_cell(j, k, z[p], z1, z2, g0, g1, g2, LG, S);
        }
      }
    }
    // post[k] = z_n[k] + LP[k]; q = lse over k, ascending, less post[0]; mle = the first k of the largest
    int64_t best = INT64_MIN, acc = 0, post0 = 0;
    int best_k = INT32_MAX;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (64 * p > 2 * j) continue;
      const int k = 64 * p + lane;
      const int64_t post = k <= 2 * j ? z[p] + m.LP[k] : INT64_MIN;
      if (post > best) best = post, best_k = k;
      const int count = 2 * j + 1 - 64 * p < 64 ? 2 * j + 1 - 64 * p : 64;
      for (int l = 0; l < count; ++l) {
        const int64_t v = __shfl(post, l);
        if (p == 0 && l == 0) acc = post0 = v;
        else acc = jg_lse(acc, v, S);
      }
    }
    for (int d = 32; d >= 1; d >>= 1) {
      const int64_t ov = __shfl_xor(best, d);
      const int ok = __shfl_xor(best_k, d);
      if (ov > best || (ov == best && ok < best_k)) best = ov, best_k = ok;
    }
    if (lane == 0) q[it] = acc - post0, mle[it] = best_k;
  }
}

__global__ __launch_bounds__(kJgBlock) void jg_site_kernel(fcsjg_sites st, int32_t n_samples, int64_t min_qual,
                                                           fcsjg_out o, int64_t* __restrict__ counts) {
  for (int64_t site = (int64_t)blockIdx.x * kJgBlock + threadIdx.x; site < st.n_sites; site += (int64_t)gridDim.x * kJgBlock) {
    const int n_alt = st.n_alt[site] < kJgAltsMax ? st.n_alt[site] : kJgAltsMax;
    int mask = 0;
    int64_t qual = 0;
    for (int i = 0; i < kJgAltsMax; ++i) {
      if (i < n_alt && o.mle[site * kJgAltsMax + i] > 0) mask |= 1 << i, qual += o.q[site * kJgAltsMax + i];
      o.ac[site * kJgAltsMax + i] = 0;
    }
    const int K = __popc(mask);
    o.qual[site] = qual, o.kept[site] = (uint8_t)mask, o.an[site] = 0, o.dp[site] = 0;
    counts[site] = mask && qual >= min_qual ? (int64_t)n_samples * ((K + 1) * (K + 2) / 2) : 0;
  }
}

// pl_off[site]: the sum of the counts before it, or -1 for a site with none; *n_pl the total.
__global__ __launch_bounds__(kJgBlock) void jg_scan_kernel(const int64_t* __restrict__ counts, int64_t n_sites, int64_t max_pl,
                                                           int64_t* __restrict__ pl_off, int64_t* __restrict__ n_pl,
                                                           int32_t* __restrict__ status) {
  __shared__ int64_t wave_sums[kJgWaves];
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  int64_t carry = 0;
  for (int64_t t0 = 0; t0 < n_sites; t0 += kJgBlock) {
    const int64_t t = t0 + (int64_t)threadIdx.x;
    const int64_t v = t < n_sites ? counts[t] : 0;
    int64_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = __shfl_up(inc, d);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    int64_t before = 0, total = 0;
    for (int k = 0; k < kJgWaves; ++k) {
      const int64_t s = wave_sums[k];
      if (k < wave) before += s;
      total += s;
    }
    __syncthreads();  // wave_sums is written again
    if (t < n_sites) pl_off[t] = v > 0 ? carry + before + inc - v : -1;
    carry += total;
  }
  if (threadIdx.x == 0) {
    *n_pl = carry;
    if (carry > max_pl) atomicOr(status, kJgStatusPl);
  }
}

__global__ __launch_bounds__(kJgBlock) void jg_geno_kernel(fcsjg_cohort c, fcsjg_sites st, fcsjg_out o,
                                                           int32_t* __restrict__ status) {
  const int64_t cells = st.n_sites * c.n_samples;
  for (int64_t i = (int64_t)blockIdx.x * kJgBlock + threadIdx.x; i < cells; i += (int64_t)gridDim.x * kJgBlock) {
    const int64_t site = i / c.n_samples;
    const int s = (int)(i - site * c.n_samples);
    const int64_t off = o.pl_off[site], r = o.src[i];
    int gt[2] = {kJgNoCall, kJgNoCall}, gq = 0;
    if (off >= 0) {
      int K;
      const uint32_t a = jg_kept(o.kept[site], &K);
      const int G = (K + 1) * (K + 2) / 2;
      const int64_t base = off + (int64_t)s * G;
      if (r >= 0) {
        const int kind = c.kind[r];
        const JgPl pl = jg_load_pl(c.pl + 6 * r, kind);
        if (pl.clamped) atomicOr(status, kJgStatusField);
        atomicAdd(reinterpret_cast<unsigned long long*>(o.dp + site), (unsigned long long)(int64_t)c.dp[r]);
        const bool called = jg_genotype(
            kind, c.alt[r], pl, a, K,
            [&](int g, int32_t v) {
              if (base + g < o.max_pl) o.pl[base + g] = v;
            },
            gt, &gq);
        if (called) {
          atomicAdd(o.an + site, 2);
          if (gt[0] > 0) atomicAdd(o.ac + site * kJgAltsMax + gt[0] - 1, 1);
          if (gt[1] > 0) atomicAdd(o.ac + site * kJgAltsMax + gt[1] - 1, 1);
        }
      } else {
        for (int g = 0; g < G; ++g)
          if (base + g < o.max_pl) o.pl[base + g] = 0;
      }
    }
    o.gt[2 * i] = (uint8_t)gt[0], o.gt[2 * i + 1] = (uint8_t)gt[1], o.gq[i] = (uint8_t)gq;
  }
}

int jg_grid(int64_t items, int cap) { return (int)std::clamp<int64_t>(items, 1, cap); }

// The workspace: a PL count per site.
size_t jg_workspace(int64_t n_sites) { return std::max<size_t>(pad256(8 * (size_t)n_sites), 256); }

template <int NP>
void launch_model(const fcsjg_cohort& c, const fcsjg_sites& st, const fcsjg_model& m, const fcsjg_out& o, hipStream_t s) {
  const int64_t waves = st.n_sites * kJgAltsMax;
  hipLaunchKernelGGL(jg_model_kernel<NP>, dim3(jg_grid((waves + kJgWaves - 1) / kJgWaves, kJgModelMaxBlocks)), dim3(kJgBlock), 0,
                     s, c, st, m, o.src, o.q, o.mle);
}

// Device pointers in every struct; n_sites > 0.
int launch_genotype(const fcsjg_cohort& c, const fcsjg_sites& st, const fcsjg_model& m, const fcsjg_out& o, char* wsp,
                    int32_t* status, hipStream_t s) {
  int64_t* counts = reinterpret_cast<int64_t*>(wsp);
  const int64_t cells = st.n_sites * c.n_samples;
  const int cell_grid = jg_grid((cells + kJgBlock - 1) / kJgBlock, kJgCellMaxBlocks);
  hipLaunchKernelGGL(jg_source_kernel, dim3(cell_grid), dim3(kJgBlock), 0, s, c, st, o.src, status);
  FCS_HIP_CHECK(hipGetLastError());
  const int cells_k = 2 * c.n_samples + 1;  // allele counts 0 .. 2 n_samples
  if (cells_k <= 64) launch_model<1>(c, st, m, o, s);
  else if (cells_k <= 64 * 2) launch_model<2>(c, st, m, o, s);
  else if (cells_k <= 64 * 3) launch_model<3>(c, st, m, o, s);
  else if (cells_k <= 64 * 5) launch_model<5>(c, st, m, o, s);
  else if (cells_k <= 64 * 9) launch_model<9>(c, st, m, o, s);
  else if (cells_k <= 64 * 17) launch_model<17>(c, st, m, o, s);
  else launch_model<33>(c, st, m, o, s);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(jg_site_kernel, dim3(jg_grid((st.n_sites + kJgBlock - 1) / kJgBlock, kJgSiteMaxBlocks)), dim3(kJgBlock), 0, s,
                     st, c.n_samples, m.min_qual, o, counts);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(jg_scan_kernel, dim3(1), dim3(kJgBlock), 0, s, counts, st.n_sites, o.max_pl, o.pl_off, o.n_pl, status);
  FCS_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(jg_geno_kernel, dim3(cell_grid), dim3(kJgBlock), 0, s, c, st, o, status);
  FCS_HIP_CHECK(hipGetLastError());
  return FCS_OK;
}

int check_scalars(const fcsjg_cohort* c, const fcsjg_sites* st, const fcsjg_model* m, const fcsjg_out* o, const char* who) {
  if (!c) return fail_invalid(who, "null cohort");
  if (!st) return fail_invalid(who, "null sites");
  if (!m) return fail_invalid(who, "null model");
  if (!o) return fail_invalid(who, "null outputs");
  if (c->n_samples < 1 || c->n_samples > FCSJG_SAMPLES_MAX)
    return fail_invalid(who, "a cohort of " + std::to_string(c->n_samples) + " samples (1 to " + std::to_string(FCSJG_SAMPLES_MAX) + ")");
  if (c->n_records < 0) return fail_invalid(who, "negative record count");
  if (st->n_sites < 0 || st->n_sites > INT32_MAX) return fail_invalid(who, "a site count of " + std::to_string(st->n_sites));
  if (o->max_pl < 0) return fail_invalid(who, "max_pl " + std::to_string(o->max_pl));
  if (!o->n_pl) return fail_invalid(who, "null PL count");
  if (st->n_sites > 0) {
    if (!c->rec_off || (c->n_records > 0 && (!c->beg || !c->end || !c->kind || !c->alt || !c->dp || !c->pl)))
      return fail_invalid(who, "null record arrays");
    if (!st->pos || !st->n_alt) return fail_invalid(who, "null site arrays");
    if (!m->S || !m->LG || !m->LP) return fail_invalid(who, "null tables");
    if (!o->q || !o->mle || !o->qual || !o->kept || !o->ac || !o->an || !o->dp || !o->pl_off || !o->src || !o->gt || !o->gq ||
        (o->max_pl > 0 && !o->pl))
      return fail_invalid(who, "null output arrays");
  }
  return FCS_OK;
}

}  // namespace

}  // namespace fcs

using namespace fcs;

extern "C" {

int fcsjg_tables(double heterozygosity, int32_t n_samples, int32_t* S, int32_t* LG, int32_t* LP) {
  const char* who = "fcsjg_tables";
  if (!S || !LG || !LP) return fail_invalid(who, "null table");
  if (n_samples < 1 || n_samples > FCSJG_SAMPLES_MAX)
    return fail_invalid(who, "a cohort of " + std::to_string(n_samples) + " samples (1 to " + std::to_string(FCSJG_SAMPLES_MAX) + ")");
  if (!(heterozygosity > 0.0 && heterozygosity < 1.0))
    return fail_invalid(who, "heterozygosity " + std::to_string(heterozygosity) + " is outside (0, 1)");
  double rest = 1.0;
  for (int k = 1; k <= 2 * n_samples; ++k) rest -= heterozygosity / k;
  if (!(rest > 0.0)) return fail_invalid(who, "heterozygosity " + std::to_string(heterozygosity) + " leaves no prior for k = 0");
  for (int i = 0; i < FCSJG_S_ROWS; ++i)
    S[i] = (int32_t)std::llround(10.0 * std::log10(1.0 + std::pow(10.0, -i / 160.0)) * 1048576.0);
  LG[0] = 0;
  for (int n = 1; n <= 4 * n_samples; ++n) LG[n] = (int32_t)std::llround(10.0 * std::log10((double)n) * 1048576.0);
  LP[0] = (int32_t)std::llround(10.0 * std::log10(rest) * 1048576.0);
  for (int k = 1; k <= 2 * n_samples; ++k) LP[k] = (int32_t)std::llround(10.0 * std::log10(heterozygosity / k) * 1048576.0);
  return FCS_OK;
}

int64_t fcsjg_workspace_bytes(int64_t n_sites, int32_t n_samples) {
  if (n_sites < 0 || n_sites > INT32_MAX || n_samples < 1 || n_samples > FCSJG_SAMPLES_MAX)
    return fail_invalid("fcsjg_workspace_bytes", std::to_string(n_sites) + " sites and " + std::to_string(n_samples) + " samples");
  return (int64_t)jg_workspace(n_sites);
}

int fcsjg_genotype_dev(int32_t device, const fcsjg_cohort* cohort, const fcsjg_sites* sites, const fcsjg_model* model,
                       const fcsjg_out* out, void* dev_workspace, int64_t workspace_bytes, int32_t* dev_status, void* stream) {
  const char* who = "fcsjg_genotype_dev";
  int rc;
  if ((rc = check_scalars(cohort, sites, model, out, who))) return rc;
  if (!dev_status || (sites->n_sites > 0 && !dev_workspace)) return fail_invalid(who, "null workspace or status");
  const int64_t need = (int64_t)jg_workspace(sites->n_sites);
  if (sites->n_sites > 0 && workspace_bytes < need)
    return fail_invalid(who, "the workspace holds " + std::to_string(workspace_bytes) + " bytes, the call needs " + std::to_string(need));
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (sites->n_sites == 0) {
    FCS_HIP_CHECK(hipMemsetAsync(out->n_pl, 0, sizeof(int64_t), s));
    return FCS_OK;
  }
  return launch_genotype(*cohort, *sites, *model, *out, static_cast<char*>(dev_workspace), dev_status, s);
}

int fcsjg_genotype(int32_t device, const fcsjg_cohort* c, const fcsjg_sites* st, const fcsjg_model* m, const fcsjg_out* o) {
  const char* who = "fcsjg_genotype";
  int rc;
  if ((rc = check_scalars(c, st, m, o, who))) return rc;
  const int64_t ns = st->n_sites, nr = c->n_records;
  const int n = c->n_samples;
  if (ns == 0) {
    *o->n_pl = 0;
    return FCS_OK;
  }
  // what the rules refuse, before any device work
  if ((rc = check_offsets(who, "record", c->rec_off, n, nr))) return rc;
  for (int s = 0; s < n; ++s)
    for (int64_t r = c->rec_off[s]; r < c->rec_off[s + 1]; ++r) {
      const std::string at = "record " + std::to_string(r - c->rec_off[s]) + " of sample " + std::to_string(s);
      if (c->beg[r] < 0 || c->end[r] <= c->beg[r]) return fail_invalid(who, at + " spans " + std::to_string(c->beg[r]) + " to " + std::to_string(c->end[r]));
      if (r > c->rec_off[s] && c->beg[r] < c->beg[r - 1])
        return fail_invalid(who, at + " at position " + std::to_string(c->beg[r]) + " follows one at " + std::to_string(c->beg[r - 1]) + ": positions decrease");
      if (c->kind[r] != FCSJG_KIND_BLOCK && c->kind[r] != FCSJG_KIND_CALL) return fail_invalid(who, at + " has kind " + std::to_string(c->kind[r]));
      if (c->alt[r] > FCSJG_ALTS_MAX) return fail_invalid(who, at + " has ALT index " + std::to_string(c->alt[r]));
      if (c->dp[r] < 0) return fail_invalid(who, at + " has DP " + std::to_string(c->dp[r]));
      for (int g = 0; g < (c->kind[r] == FCSJG_KIND_BLOCK ? 3 : 6); ++g)
        if (c->pl[6 * r + g] < 0 || c->pl[6 * r + g] > FCSJG_PL_MAX)
          return fail_invalid(who, at + " has a PL of " + std::to_string(c->pl[6 * r + g]) + " (0 to " + std::to_string(FCSJG_PL_MAX) + ")");
    }
  for (int64_t k = 0; k < ns; ++k) {
    if (st->pos[k] < 0 || (k > 0 && st->pos[k] <= st->pos[k - 1]))
      return fail_invalid(who, "site " + std::to_string(k) + " at position " + std::to_string(st->pos[k]) + ": positions do not ascend");
    if (st->n_alt[k] < 1 || st->n_alt[k] > FCSJG_ALTS_MAX)
      return fail_invalid(who, "site " + std::to_string(k) + " has " + std::to_string(st->n_alt[k]) + " ALTs (1 to " + std::to_string(FCSJG_ALTS_MAX) + ")");
  }
  if ((rc = device_ok(device))) return rc;
  FCS_SET_DEVICE((device));
  const size_t NR = (size_t)nr, NS = (size_t)ns, cells = NS * (size_t)n;
  const int64_t cap = std::min<int64_t>(o->max_pl, (int64_t)cells * FCSJG_GENOTYPES_MAX);
  Arena A;
  const size_t ooff = A.add(8 * ((size_t)n + 1)), obeg = A.add(4 * NR), oend = A.add(4 * NR), okind = A.add(NR), oalt = A.add(NR),
               odp = A.add(4 * NR), opl = A.add(24 * NR), opos = A.add(4 * NS), onalt = A.add(NS), oS = A.add(4 * FCSJG_S_ROWS),
               oLG = A.add(4 * (4 * (size_t)n + 1)), oLP = A.add(4 * (2 * (size_t)n + 1));
  const size_t in_bytes = A.total;
  const size_t otail = A.add(16);  // n_pl, status
  const size_t host_bytes = A.total;
  const size_t dq = A.add(8 * NS * 6), dmle = A.add(4 * NS * 6), dqual = A.add(8 * NS), dkept = A.add(NS), dac = A.add(4 * NS * 6),
               dan = A.add(4 * NS), ddp = A.add(8 * NS), dploff = A.add(8 * NS), dsrc = A.add(8 * cells), dgt = A.add(2 * cells),
               dgq = A.add(cells), dplv = A.add(4 * (size_t)cap), dws = A.add(jg_workspace(ns));
  CallSession S;
  if ((rc = call_session_acquire(device, host_bytes, A.total, S))) return rc;
  CallLease lease{S};
  std::memcpy(S.host + ooff, c->rec_off, 8 * ((size_t)n + 1));
  if (NR) {
    std::memcpy(S.host + obeg, c->beg, 4 * NR), std::memcpy(S.host + oend, c->end, 4 * NR);
    std::memcpy(S.host + okind, c->kind, NR), std::memcpy(S.host + oalt, c->alt, NR);
    std::memcpy(S.host + odp, c->dp, 4 * NR), std::memcpy(S.host + opl, c->pl, 24 * NR);
  }
  std::memcpy(S.host + opos, st->pos, 4 * NS), std::memcpy(S.host + onalt, st->n_alt, NS);
  std::memcpy(S.host + oS, m->S, 4 * FCSJG_S_ROWS), std::memcpy(S.host + oLG, m->LG, 4 * (4 * (size_t)n + 1));
  std::memcpy(S.host + oLP, m->LP, 4 * (2 * (size_t)n + 1));
  auto dev = [&](size_t off) { return S.dev + off; };
  fcsjg_cohort dc = *c;
  dc.rec_off = reinterpret_cast<const int64_t*>(dev(ooff)), dc.beg = reinterpret_cast<const int32_t*>(dev(obeg));
  dc.end = reinterpret_cast<const int32_t*>(dev(oend)), dc.kind = reinterpret_cast<const uint8_t*>(dev(okind));
  dc.alt = reinterpret_cast<const uint8_t*>(dev(oalt)), dc.dp = reinterpret_cast<const int32_t*>(dev(odp));
  dc.pl = reinterpret_cast<const int32_t*>(dev(opl));
  fcsjg_sites ds{ns, reinterpret_cast<const int32_t*>(dev(opos)), reinterpret_cast<const uint8_t*>(dev(onalt))};
  fcsjg_model dm{reinterpret_cast<const int32_t*>(dev(oS)), reinterpret_cast<const int32_t*>(dev(oLG)),
                 reinterpret_cast<const int32_t*>(dev(oLP)), m->min_qual};
  fcsjg_out d{};
  d.q = reinterpret_cast<int64_t*>(dev(dq)), d.mle = reinterpret_cast<int32_t*>(dev(dmle)), d.qual = reinterpret_cast<int64_t*>(dev(dqual));
  d.kept = reinterpret_cast<uint8_t*>(dev(dkept)), d.ac = reinterpret_cast<int32_t*>(dev(dac)), d.an = reinterpret_cast<int32_t*>(dev(dan));
  d.dp = reinterpret_cast<int64_t*>(dev(ddp)), d.pl_off = reinterpret_cast<int64_t*>(dev(dploff)), d.src = reinterpret_cast<int64_t*>(dev(dsrc));
  d.gt = reinterpret_cast<uint8_t*>(dev(dgt)), d.gq = reinterpret_cast<uint8_t*>(dev(dgq)), d.pl = reinterpret_cast<int32_t*>(dev(dplv));
  d.max_pl = cap, d.n_pl = reinterpret_cast<int64_t*>(dev(otail));
  int32_t* status = reinterpret_cast<int32_t*>(dev(otail) + 8);
  FCS_HIP_CHECK(hipMemcpyAsync(S.dev, S.host, in_bytes, hipMemcpyHostToDevice, S.s));
  FCS_HIP_CHECK(hipMemsetAsync(dev(otail), 0, 16, S.s));
  if ((rc = launch_genotype(dc, ds, dm, d, dev(dws), status, S.s))) return rc;
  FCS_HIP_CHECK(hipMemcpyAsync(S.host + otail, dev(otail), 16, hipMemcpyDeviceToHost, S.s));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  int64_t n_pl;
  int32_t stw;
  std::memcpy(&n_pl, S.host + otail, sizeof n_pl);
  std::memcpy(&stw, S.host + otail + 8, sizeof stw);
  if ((stw & FCSJG_STATUS_PL) || n_pl > o->max_pl)
    return fail_invalid(who, "the sites written have " + std::to_string(n_pl) + " PLs, max_pl is " + std::to_string(o->max_pl));
  if (stw) return fail(FCS_ERR_DEVICE, "[E::fcsjg_genotype] the device clamped a checked field (status " + std::to_string(stw) + ")");
  auto back = [&](void* to, size_t off, size_t bytes) { return bytes ? hipMemcpyAsync(to, dev(off), bytes, hipMemcpyDeviceToHost, S.s) : hipSuccess; };
  FCS_HIP_CHECK(back(o->q, dq, 8 * NS * 6));
  FCS_HIP_CHECK(back(o->mle, dmle, 4 * NS * 6));
  FCS_HIP_CHECK(back(o->qual, dqual, 8 * NS));
  FCS_HIP_CHECK(back(o->kept, dkept, NS));
  FCS_HIP_CHECK(back(o->ac, dac, 4 * NS * 6));
  FCS_HIP_CHECK(back(o->an, dan, 4 * NS));
  FCS_HIP_CHECK(back(o->dp, ddp, 8 * NS));
  FCS_HIP_CHECK(back(o->pl_off, dploff, 8 * NS));
  FCS_HIP_CHECK(back(o->src, dsrc, 8 * cells));
  FCS_HIP_CHECK(back(o->gt, dgt, 2 * cells));
  FCS_HIP_CHECK(back(o->gq, dgq, cells));
  FCS_HIP_CHECK(back(o->pl, dplv, 4 * (size_t)n_pl));
  FCS_HIP_CHECK(hipStreamSynchronize(S.s));
  *o->n_pl = n_pl;
  return FCS_OK;
}

}  // extern "C"
