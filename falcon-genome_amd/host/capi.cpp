// extern "C" hooks of libfcsgenome.so for the Python tests (tests/test_host_*.py):
// the host pieces with exact expected outputs — GATK read preparation,
// interval partitioning, BGZF, BAM record coding, BAI/TBI building, the
// executor's stage/error semantics.  Not part of the hot-path ABI (include/fcship.h).
#include <cstring>
#include <functional>
#include <memory>
#include <string>

#include "bam.h"
#include "bam_input.h"
#include "caller.h"
#include "bgzf.h"
#include "bqsr.h"
#include "depth.h"
#include "ug.h"
#include "common.h"
#include "config.h"
#include "executor.h"
#include "fasta.h"
#include "fmindex.h"
#include "gatk_prep.h"
#include "gpu_seed.h"
#include "seedext.h"
#include "aligner.h"
#include "indel.h"
#include "intervals.h"
#include "joint.h"
#include "markdup.h"
#include "minimizer.h"
#include "pileup.h"
#include "sample_sheet.h"
#include "vcf.h"

using namespace fcsg;

namespace {
thread_local std::string g_err;
int guard(const std::function<void()>& fn) {
  try {
    fn();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
int copy_out(const std::string& s, char* buf, int cap) {
  if ((int)s.size() + 1 > cap) return -(int)s.size() - 1;
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return (int)s.size();
}
}  // namespace

extern "C" {

const char* fcsg_last_error() { return g_err.c_str(); }

int fcsg_prepare_read(const char* bases, const uint8_t* quals, int len, const char* bi, const char* bd, int mapq,
                      int threshold, int pcr_model, uint8_t* bq, uint8_t* iq, uint8_t* dq, uint8_t* gcp) {
  return guard([&] {
    PreparedRead pr;
    gatk_prepare_read(std::string(bases, len), std::vector<uint8_t>(quals, quals + len), bi ? std::string(bi) : "",
                      bd ? std::string(bd) : "", mapq, pr, threshold, (PcrIndelModel)pcr_model);
    std::memcpy(bq, pr.base_q.data(), len);
    std::memcpy(iq, pr.ins_q.data(), len);
    std::memcpy(dq, pr.del_q.data(), len);
    std::memcpy(gcp, pr.gcp.data(), len);
  });
}

// "sample\tfastq1\tfastq2\trg\tplatform\tlibrary\n" lines of a sample sheet
// (file or FASTQ folder), samples in name order, read groups in sheet order.
int fcsg_sample_sheet(const char* path, char* buf, int cap) {
  int rc = 0;
  const int g = guard([&] {
    std::string s;
    for (const auto& [sample, list] : read_sample_sheet(path))
      for (const SampleDetails& d : list)
        s += sample + "\t" + d.fastqR1 + "\t" + d.fastqR2 + "\t" + d.ReadGroup + "\t" + d.Platform + "\t" +
             d.LibraryID + "\n";
    rc = copy_out(s, buf, cap);
  });
  return g ? g : rc;
}

// merge_sorted_bams (align's per-sample merge of read-group BAMs).
int fcsg_merge_bams(const char* const* inputs, int n, const char* output) {
  return guard([&] { merge_sorted_bams(std::vector<std::string>(inputs, inputs + n), output); });
}

// "shard\tchrom\tlb\tub\n" lines of the init_contig_intv partition of a .dict.
int fcsg_partition_dict(const char* dict_path, int ncontigs, int skip_pseudo, char* buf, int cap) {
  int rc = 0;
  const int g = guard([&] {
    const auto parts = partition_contigs(read_dict(dict_path), ncontigs, skip_pseudo != 0);
    std::string s;
    for (size_t k = 0; k < parts.size(); ++k)
      for (const Interval& iv : parts[k])
        s += std::to_string(k) + "\t" + iv.chrom + "\t" + std::to_string(iv.lb) + "\t" + std::to_string(iv.ub) + "\n";
    rc = copy_out(s, buf, cap);
  });
  return g ? g : rc;
}

// BamInput::merge_region: "bam1,bam2,...\n<region file>\n" of shard `contig`.
int fcsg_bam_input_shard(const char* path, int contig, int ncontigs, const char* temp_dir, char* buf, int cap) {
  int rc = 0;
  const int g = guard([&] {
    const BamShard sh = BamInput(path).merge_region(contig, ncontigs, temp_dir);
    std::string s;
    for (size_t i = 0; i < sh.bams.size(); ++i) s += (i ? "," : "") + sh.bams[i];
    s += "\n" + sh.region + "\n";
    rc = copy_out(s, buf, cap);
  });
  return g ? g : rc;
}

// read_regions of each path, intersected when several: "chrom\tlb\tub\n" lines.
int fcsg_intersect_regions(const char* const* paths, int n, char* buf, int cap) {
  int rc = 0;
  const int g = guard([&] {
    std::vector<std::vector<Interval>> sets;
    for (int i = 0; i < n; ++i) sets.push_back(read_regions(paths[i]));
    const auto out = sets.size() == 1 ? sets[0] : intersect_interval_sets(sets);
    std::string s;
    for (const Interval& iv : out) s += iv.chrom + "\t" + std::to_string(iv.lb) + "\t" + std::to_string(iv.ub) + "\n";
    rc = copy_out(s, buf, cap);
  });
  return g ? g : rc;
}

int fcsg_gvcf_band(int gq) { return gvcf_band(gq); }

// SMEM seeding on an FMD-index of the given contigs (codes 0..4): seeds of q
// (bwa mem_collect_intv; max_mem_intv 0 skips its third round), out = {qb, qe, occurrences} per SMEM and
// loc = {contig, offset, reverse} of every occurrence (at most loc_cap rows,
// SMEM by SMEM, each SMEM's occurrences in suffix-array order).  Returns the
// SMEM count, or < 0 on error.
// sa_intv: the index's SA sampling; index_path non-empty: the index is saved
// there and the query runs on the file mapped back (FmdIndex::load).
int fcsg_fmd_smems(const uint8_t* ref, const int64_t* clen, int ncontig, const uint8_t* q, int qlen, int min_len,
                   int split_len, int split_width, int max_mem_intv, int32_t* out, int cap, int64_t* loc,
                   int loc_cap, int sa_intv, const char* index_path) {
  int n = -1;
  const int rc = guard([&] {
    std::vector<std::vector<uint8_t>> cs;
    int64_t o = 0;
    for (int i = 0; i < ncontig; ++i) {
      cs.emplace_back(ref + o, ref + o + clen[i]);
      o += clen[i];
    }
    std::unique_ptr<FmdIndex> built = std::make_unique<FmdIndex>(cs, sa_intv), mapped;
    if (index_path && *index_path) {
      built->save(index_path);
      built.reset();
      mapped = FmdIndex::load(index_path, cs);
      if (!mapped) throw internalError("saved FMD-index did not load");
    }
    const FmdIndex& fmd = mapped ? *mapped : *built;
    std::vector<BiInterval> v;
    fmd.collect(q, qlen, min_len, split_len, split_width, max_mem_intv, v);
    if ((int)v.size() > cap) throw invalidParam("fcsg_fmd_smems: capacity");
    int64_t nl = 0;
    for (size_t i = 0; i < v.size(); ++i) {
      out[3 * i] = v[i].qb, out[3 * i + 1] = v[i].qe, out[3 * i + 2] = (int32_t)v[i].s;
      for (int64_t j = 0; j < v[i].s && nl < loc_cap; ++j, ++nl) {
        int c;
        int64_t off;
        bool rev;
        fmd.locate(v[i], j, c, off, rev);
        loc[3 * nl] = c, loc[3 * nl + 1] = off, loc[3 * nl + 2] = rev;
      }
    }
    n = (int)v.size();
  });
  return rc < 0 ? rc : n;
}

int fcsg_fmd_seeds(const uint8_t* ref, const int64_t* clen, int ncontig, const uint8_t* q, const int64_t* qoff,
                   const int32_t* qlen, int n, int min_len, int split_len, int split_width, int max_mem_intv,
                   int max_occ, int sa_intv, const char* index_path, int mode, int max_mems, int max_steps,
                   int64_t start_mem_cap, int64_t start_row_cap, int64_t* mems, int64_t* mem_off, int32_t* n_mems,
                   int64_t mem_cap, int64_t* loc, int64_t* loc_off, int32_t* n_loc, int64_t loc_cap, int64_t* stats);

// The aligner's seeding of a batch of reads (codes 0..4, read r at q[qoff[r] ..
// qoff[r] + qlen[r])) on an FMD-index of the given contigs, on the host index
// (gpu 0: FmdIndex::collect / locate) or through the device entry points (gpu
// 1: host/gpu_seed.h on device 0).  Per read r: n_mems[r] SMEMs {qb, qe, s, k,
// l} at mems + 5 * mem_off[r] in collect's order, and n_loc[r] located
// occurrences {contig, offset, reverse} at loc + 3 * loc_off[r], those
// seed_read samples (at most max_occ per SMEM); mem_off / loc_off are the
// prefix sums the call writes (n + 1 entries); a total beyond mem_cap /
// loc_cap is an error.  *fallback = reads the device handed back to the host.
// sa_intv / index_path as fcsg_fmd_smems.
int fcsg_fmd_seed_batch(const uint8_t* ref, const int64_t* clen, int ncontig, const uint8_t* q, const int64_t* qoff,
                        const int32_t* qlen, int n, int min_len, int split_len, int split_width, int max_mem_intv,
                        int max_occ, int sa_intv, const char* index_path, int gpu, int max_mems, int64_t* mems,
                        int64_t* mem_off, int32_t* n_mems, int64_t mem_cap, int64_t* loc, int64_t* loc_off,
                        int32_t* n_loc, int64_t loc_cap, int64_t* fallback) {
  int64_t stats[3] = {0, 0, 0};
  const int rc = fcsg_fmd_seeds(ref, clen, ncontig, q, qoff, qlen, n, min_len, split_len, split_width, max_mem_intv,
                                max_occ, sa_intv, index_path, gpu ? 1 : 0, max_mems, 0, 0, 0, mems, mem_off, n_mems,
                                mem_cap, loc, loc_off, n_loc, loc_cap, stats);
  if (rc == 0) *fallback = stats[0];
  return rc;
}

// fcsg_fmd_seed_batch with the path chosen by mode: 0 the host index, 1 the
// two-call device path (fcs_fmd_collect, fcs_fmd_locate), 2 the fused call
// (fcs_fmd_seed) with the device's LF-step cap max_steps (0: its default) and
// the capacities start_mem_cap / start_row_cap for its first call (0: the
// aligner's).  stats = {reads collected on the host, rows located on the host,
// fused calls repeated with more room}.
int fcsg_fmd_seeds(const uint8_t* ref, const int64_t* clen, int ncontig, const uint8_t* q, const int64_t* qoff,
                   const int32_t* qlen, int n, int min_len, int split_len, int split_width, int max_mem_intv,
                   int max_occ, int sa_intv, const char* index_path, int mode, int max_mems, int max_steps,
                   int64_t start_mem_cap, int64_t start_row_cap, int64_t* mems, int64_t* mem_off, int32_t* n_mems,
                   int64_t mem_cap, int64_t* loc, int64_t* loc_off, int32_t* n_loc, int64_t loc_cap, int64_t* stats) {
  return guard([&] {
    std::vector<std::vector<uint8_t>> cs;
    int64_t o = 0;
    for (int i = 0; i < ncontig; ++i) {
      cs.emplace_back(ref + o, ref + o + clen[i]);
      o += clen[i];
    }
    std::unique_ptr<FmdIndex> built = std::make_unique<FmdIndex>(cs, sa_intv), mapped;
    if (index_path && *index_path) {
      built->save(index_path);
      built.reset();
      mapped = FmdIndex::load(index_path, cs);
      if (!mapped) throw internalError("saved FMD-index did not load");
    }
    const FmdIndex& fmd = mapped ? *mapped : *built;
    SeedParams P;
    P.min_len = min_len, P.split_len = split_len, P.split_width = split_width, P.max_mem_intv = max_mem_intv;
    P.max_occ = max_occ, P.max_mems = max_mems;
    P.max_steps = max_steps, P.mem_cap = start_mem_cap, P.row_cap = start_row_cap;
    if (max_occ < 1) throw invalidParam("fcsg_fmd_seed_batch: max_occ");
    if (mode < 0 || mode > 2) throw invalidParam("fcsg_fmd_seeds: mode");
    SeedBatch sb;
    if (mode) {
      if (!gpu_seed_available()) throw internalError("fcsg_fmd_seed_batch: libfcship has no fcs_fmd_* entry points");
      if (mode == 2 && !gpu_seed_fused_available()) throw internalError("fcsg_fmd_seeds: libfcship has no fcs_fmd_seed");
      FmdDeviceCopies dev(fmd);
      std::vector<const uint8_t*> qp(n);
      for (int r = 0; r < n; ++r) qp[r] = q + qoff[r];
      gpu_seed_batch(fmd, dev.get(0), qp.data(), qlen, (size_t)n, P, 4, sb, mode == 2);
    } else {
      sb.mems.resize(n);
      for (int r = 0; r < n; ++r)
        fmd.collect(q + qoff[r], qlen[r], min_len, split_len, split_width, max_mem_intv, sb.mems[r]);
    }
    const TextMap map(cs);
    int64_t nm = 0, nl = 0;
    for (int r = 0; r < n; ++r) {
      mem_off[r] = nm, loc_off[r] = nl;
      const int64_t* pos = mode ? sb.pos_of((size_t)r) : nullptr;  // null: a read of the host's
      const BiInterval* rm = mode ? sb.mems_of((size_t)r) : sb.mems[r].data();
      const size_t rn = mode ? sb.n_mems_of((size_t)r) : sb.mems[r].size();
      for (size_t i = 0; i < rn; ++i) {
        const BiInterval& m = rm[i];
        if (nm >= mem_cap) throw invalidParam("fcsg_fmd_seed_batch: SMEM capacity");
        int64_t* w = mems + 5 * nm++;
        w[0] = m.qb, w[1] = m.qe, w[2] = m.s, w[3] = m.k, w[4] = m.l;
        const int64_t step = m.s > max_occ ? m.s / max_occ : 1;
        for (int64_t j = 0, kept = 0; j < m.s && kept < max_occ; j += step, ++kept) {
          if (nl >= loc_cap) throw invalidParam("fcsg_fmd_seed_batch: location capacity");
          int c;
          int64_t off;
          bool rev;
          if (pos) map.locate(*pos++, m.qe - m.qb, c, off, rev);
          else fmd.locate(m, j, c, off, rev);
          int64_t* l = loc + 3 * nl++;
          l[0] = c, l[1] = off, l[2] = rev;
        }
      }
      n_mems[r] = (int32_t)(nm - mem_off[r]);
      n_loc[r] = (int32_t)(nl - loc_off[r]);
    }
    mem_off[n] = nm, loc_off[n] = nl;
    stats[0] = sb.host_reads, stats[1] = sb.host_rows, stats[2] = sb.retries;
  });
}

// Host seeding rates for tools/bench_seed.py: FmdIndex::collect of every read,
// then FmdIndex::locate of the occurrences seed_read samples, each phase on
// `threads` threads (parallel_for, as align_batch runs them) and timed alone.
// out = {collect seconds, locate seconds}, counts = {SMEMs, rows located}.
int fcsg_fmd_host_rates(const uint8_t* ref, const int64_t* clen, int ncontig, const uint8_t* q, const int64_t* qoff,
                        const int32_t* qlen, int n, int min_len, int split_len, int split_width, int max_mem_intv,
                        int max_occ, int sa_intv, int threads, double* out, int64_t* counts) {
  return guard([&] {
    std::vector<std::vector<uint8_t>> cs;
    int64_t o = 0;
    for (int i = 0; i < ncontig; ++i) {
      cs.emplace_back(ref + o, ref + o + clen[i]);
      o += clen[i];
    }
    const FmdIndex fmd(cs, sa_intv);
    std::vector<std::vector<BiInterval>> mems(n);
    const uint64_t t0 = now_us();
    parallel_for((size_t)n, threads, [&](size_t r) {
      fmd.collect(q + qoff[r], qlen[r], min_len, split_len, split_width, max_mem_intv, mems[r]);
    });
    const uint64_t t1 = now_us();
    std::vector<int64_t> rows(n, 0);
    parallel_for((size_t)n, threads, [&](size_t r) {
      for (const BiInterval& m : mems[r]) {
        const int64_t step = m.s > max_occ ? m.s / max_occ : 1;
        for (int64_t j = 0, kept = 0; j < m.s && kept < max_occ; j += step, ++kept) {
          int c;
          int64_t off;
          bool rev;
          fmd.locate(m, j, c, off, rev);
          ++rows[r];
        }
      }
    });
    out[0] = (t1 - t0) / 1e6;
    out[1] = (now_us() - t1) / 1e6;
    counts[0] = counts[1] = 0;
    for (int r = 0; r < n; ++r) counts[0] += (int64_t)mems[r].size(), counts[1] += rows[r];
  });
}

// The arrays of the FMD-index of the given contigs, as the fcs_fmd_* entry
// points of libfcship take them (FmdIndex::view): sizes = {n_occ_words, n_rows,
// n_sa, n_special, flen}; the arrays are filled when non-null (call once for
// the sizes, then with buffers of those sizes; C6 holds 6 entries).
int fcsg_fmd_index_arrays(const uint8_t* ref, const int64_t* clen, int ncontig, int sa_intv, int64_t* sizes,
                          uint64_t* occ, int64_t* C6, uint64_t* sa, int64_t* special_rows, int64_t* special_sa) {
  return guard([&] {
    std::vector<std::vector<uint8_t>> cs;
    int64_t o = 0;
    for (int i = 0; i < ncontig; ++i) {
      cs.emplace_back(ref + o, ref + o + clen[i]);
      o += clen[i];
    }
    const FmdIndex fmd(cs, sa_intv);
    const FmdView v = fmd.view();
    sizes[0] = v.n_occ_words, sizes[1] = v.n_rows, sizes[2] = v.n_sa, sizes[3] = v.n_special, sizes[4] = v.flen;
    if (occ) std::copy(v.occ, v.occ + v.n_occ_words, occ);
    if (C6) std::copy(v.C, v.C + 6, C6);
    if (sa) std::copy(v.sa, v.sa + v.n_sa, sa);
    for (int64_t i = 0; i < v.n_special; ++i) {
      if (special_rows) special_rows[i] = v.special[2 * i];
      if (special_sa) special_sa[i] = v.special[2 * i + 1];
    }
  });
}

// bwa's seed-extension protocol (host/seedext.h) over n seeds on one reference
// sequence (codes 0..4), each with its chain's window (win_lo / win_hi, or
// null / -1 for the seed's own); per job out_i = {qb, qe, score, truesc, w, gscore, gw},
// out_r = {rb, re}, the CIGAR (ksw ops) in cig[cig_off[i] ...] (ncig[i] ops).
int fcsg_extend_seeds(int n, const uint8_t* qbuf, const int64_t* qoff, const int32_t* qlen, const uint8_t* ref,
                      int64_t rlen, const int32_t* seed_q, const int64_t* seed_r, const int32_t* seed_len, int w,
                      int pen_clip5, int pen_clip3, int gpu, int32_t* out_i, int64_t* out_r, uint32_t* cig,
                      const int64_t* cig_off, const int32_t* cig_cap, int32_t* ncig, const int64_t* win_lo,
                      const int64_t* win_hi) {
  return guard([&] {
    std::vector<SeedJob> jobs(n);
    for (int i = 0; i < n; ++i) {
      if (win_lo) jobs[i].win_lo = win_lo[i];
      if (win_hi) jobs[i].win_hi = win_hi[i];
      jobs[i].q = qbuf + qoff[i];
      jobs[i].qlen = qlen[i];
      jobs[i].ref = ref;
      jobs[i].rlen = rlen;
      jobs[i].seed_q = seed_q[i];
      jobs[i].seed_r = seed_r[i];
      jobs[i].seed_len = seed_len[i];
    }
    fcs_bsw_params P;
    fcs_bsw_params_default(&P);
    SeedExtOptions so;
    so.w = w;
    so.pen_clip5 = pen_clip5;
    so.pen_clip3 = pen_clip3;
    so.gpu = gpu;
    std::vector<SeedAln> res;
    SeedExtStats st;
    extend_seeds(jobs, P, so, res, st);
    for (int i = 0; i < n; ++i) {
      const SeedAln& x = res[i];
      int32_t* o = out_i + 7 * (int64_t)i;
      o[0] = x.qb, o[1] = x.qe, o[2] = x.score, o[3] = x.truesc, o[4] = x.w, o[5] = x.gscore, o[6] = x.gw;
      out_r[2 * i] = x.rb;
      out_r[2 * i + 1] = x.re;
      if ((int64_t)x.cigar.size() > cig_cap[i]) throw invalidParam("fcsg_extend_seeds: CIGAR capacity");
      std::copy(x.cigar.begin(), x.cigar.end(), cig + cig_off[i]);
      ncig[i] = (int32_t)x.cigar.size();
    }
  });
}
int fcsg_tandem_repeat_units(const char* bases, int offset) { return tandem_repeat_units(bases, offset); }
void fcsg_tandem_repeat_runs(const char* bases, int n, uint8_t* out) { tandem_repeat_runs(bases, n, out); }
int fcsg_pcr_indel_cap(int repeat_len, int model) { return pcr_indel_cap(repeat_len, (PcrIndelModel)model); }

int fcsg_bgzf_compress_file(const char* in, const char* out) {
  return guard([&] { bgzip_file(in, out); });
}

// Decompress a BGZF file with the library's reader (tests compare with Python's gzip).
int fcsg_bgzf_decompress_file(const char* in, const char* out) {
  return guard([&] {
    BgzfReader r(in);
    std::string all;
    char buf[1 << 16];
    for (size_t n; (n = r.read(buf, sizeof buf)) > 0;) all.append(buf, n);
    write_file(out, all);
  });
}

// BAM → SAM-like text (one line per record) with the library's reader.
int fcsg_bam_to_text(const char* bam, const char* out) {
  return guard([&] {
    BamReader r(bam);
    std::string s;
    for (size_t i = 0; i < r.header().names.size(); ++i)
      s += "@SQ\t" + r.header().names[i] + "\t" + std::to_string(r.header().lengths[i]) + "\n";
    BamRecord rec;
    while (r.next(rec)) {
      std::string q;
      for (uint8_t x : rec.qual) q += (char)(x + 33);
      std::string md;
      int64_t nm = -1;
      rec.get_aux_string("MD", md);
      rec.get_aux_int("NM", nm);
      s += rec.name + "\t" + std::to_string(rec.flag) + "\t" + std::to_string(rec.ref_id) + "\t" +
           std::to_string(rec.pos) + "\t" + std::to_string(rec.mapq) + "\t" + cigar_string(rec.cigar) + "\t" + rec.seq +
           "\t" + (q.empty() ? "*" : q) + "\t" + md + "\t" + std::to_string(nm) + "\n";
    }
    write_file(out, s);
  });
}

// SAM-like text (name flag ref_id pos mapq cigar seq qual; leading '@' lines
// are header lines) → BAM with the library's writer.
int fcsg_text_to_bam(const char* text, const char* bam, const char* names_csv, const char* lengths_csv) {
  return guard([&] {
    BamHeader h;
    std::string nm = names_csv, ln = lengths_csv;
    for (size_t p = 0; p < nm.size();) {
      const size_t e = std::min(nm.find(',', p), nm.size());
      h.names.push_back(nm.substr(p, e - p));
      p = e + 1;
    }
    for (size_t p = 0; p < ln.size();) {
      const size_t e = std::min(ln.find(',', p), ln.size());
      h.lengths.push_back(std::stoll(ln.substr(p, e - p)));
      p = e + 1;
    }
    for (size_t i = 0; i < h.names.size(); ++i)
      h.text += "@SQ\tSN:" + h.names[i] + "\tLN:" + std::to_string(h.lengths[i]) + "\n";
    std::string body = read_file(text);
    while (!body.empty() && body[0] == '@') {  // leading header lines (@RG, @PG) join the header
      const size_t e = std::min(body.find('\n'), body.size());
      h.text += body.substr(0, e) + "\n";
      body.erase(0, e + 1);
    }
    BamWriter w(bam, h);
    size_t p = 0;
    while (p < body.size()) {
      const size_t e = std::min(body.find('\n', p), body.size());
      const std::string line = body.substr(p, e - p);
      p = e + 1;
      if (line.empty()) continue;
      std::vector<std::string> f;
      for (size_t a = 0; a <= line.size();) {
        const size_t b = std::min(line.find('\t', a), line.size());
        f.push_back(line.substr(a, b - a));
        a = b + 1;
      }
      if (f.size() < 8) throw formatError("text record needs 8 fields");
      BamRecord r;
      r.name = f[0];
      r.flag = (uint16_t)std::stoi(f[1]);
      r.ref_id = std::stoi(f[2]);
      r.pos = std::stoi(f[3]);
      r.mapq = (uint8_t)std::stoi(f[4]);
      r.cigar = parse_cigar(f[5]);
      r.seq = f[6];
      if (f[7] != "*")
        for (char c : f[7]) r.qual.push_back((uint8_t)(c - 33));
      w.write(r);
    }
    w.close();
  });
}

// mark_duplicates_host over a flat batch (the layout of include/fcsdup.h):
// dup[n] and stats = {examined, pairs, fragments, duplicate records}.
int fcsg_markdup(int64_t n, const uint16_t* flag, const int32_t* ref_id, const int32_t* pos, const int32_t* mate,
                 const int32_t* lib, const uint32_t* cigar, const int64_t* cigar_off, const uint8_t* qual,
                 const int64_t* qual_off, int32_t n_ref, int32_t n_lib, uint8_t* dup, int64_t* stats) {
  return guard([&] {
    fcsdup_batch b;
    b.n = n;
    b.flag = flag, b.ref_id = ref_id, b.pos = pos, b.mate = mate, b.lib = lib;
    b.cigar = cigar, b.cigar_off = cigar_off, b.n_cigar = n > 0 ? cigar_off[n] : 0;
    b.qual = qual, b.qual_off = qual_off, b.n_qual = n > 0 ? qual_off[n] : 0;
    b.n_ref = n_ref, b.n_lib = n_lib;
    const MarkdupStats st = mark_duplicates_host(b, dup);
    stats[0] = st.examined, stats[1] = st.pairs, stats[2] = st.fragments, stats[3] = st.duplicates;
  });
}

// The host statement of base quality recalibration (bqsr.h) over a flat batch
// (include/fcsbq.h) and a flat reference: counts added to ctx / cyc, the
// finalised tables, the applied qualities, and the report written and read
// (names: the read groups' labels, one per line).
int fcsg_bqsr_count(const fcsbq_batch* b, const uint8_t* ref_bases, const int64_t* ref_off, int32_t n_ref,
                    const uint64_t* known, int32_t n_rg, int threads, int64_t* ctx, int64_t* cyc) {
  return guard([&] {
    BqRefView ref;
    ref.bases = ref_bases, ref.ref_off = ref_off, ref.n_ref = n_ref, ref.known = known;
    bqsr_count_host(ref, *b, n_rg, ctx, cyc, threads);
  });
}

int fcsg_bqsr_finalize(int32_t n_rg, const int64_t* ctx, const int64_t* cyc, double* base, double* dctx, double* dcyc) {
  return guard([&] {
    const BqTables t = bqsr_finalize(n_rg, ctx, cyc);
    std::memcpy(base, t.base.data(), 8 * t.base.size());
    std::memcpy(dctx, t.dctx.data(), 8 * t.dctx.size());
    std::memcpy(dcyc, t.dcyc.data(), 8 * t.dcyc.size());
  });
}

int fcsg_bqsr_apply(const fcsbq_batch* b, int32_t n_rg, const double* base, const double* dctx, const double* dcyc,
                    int threads, uint8_t* out_qual) {
  return guard([&] {
    BqTables t;
    t.n_rg = n_rg;
    t.base.assign(base, base + (size_t)n_rg * FCSBQ_NQ);
    t.dctx.assign(dctx, dctx + (size_t)n_rg * kBqCtxCells);
    t.dcyc.assign(dcyc, dcyc + (size_t)n_rg * kBqCycCells);
    bqsr_apply_host(*b, t, out_qual, threads);
  });
}

namespace {
std::vector<std::string> split_lines(const char* s) {
  std::vector<std::string> out;
  std::string cur;
  for (; *s; ++s)
    if (*s == '\n') out.push_back(cur), cur.clear();
    else cur += *s;
  if (!cur.empty()) out.push_back(cur);
  return out;
}
}  // namespace

int fcsg_bqsr_report(int32_t n_rg, const int64_t* ctx, const int64_t* cyc, const char* names, char* buf, int cap) {
  int rc = 0;
  const int g = guard([&] { rc = copy_out(bqsr_report_text(n_rg, ctx, cyc, split_lines(names)), buf, cap); });
  return g ? g : rc;
}

int fcsg_bqsr_report_parse(const char* text, const char* names, int64_t* ctx, int64_t* cyc) {
  return guard([&] {
    std::vector<int64_t> c, y;
    bqsr_report_parse(text, split_lines(names), c, y);
    std::memcpy(ctx, c.data(), 8 * c.size());
    std::memcpy(cyc, y.data(), 8 * y.size());
  });
}

// The host statement of depth of coverage (depth.h) over a flat batch and a
// window (include/fcsdp.h): depths added to depth[len], and the statistics of
// a window's pieces.
int fcsg_depth_count(const fcsdp_batch* b, const fcsdp_params* prm, const fcsdp_window* w, int threads, uint32_t* depth) {
  return guard([&] { depth_count_host(*b, *prm, *w, depth, threads); });
}

int fcsg_depth_stats(const uint32_t* depth, const uint64_t* bitmap, int64_t len, const fcsdp_piece* pieces, int64_t n_pieces,
                     int32_t n_long, int threads, uint64_t* hist, uint64_t* long_hist, fcsdp_summary* summary) {
  return guard([&] { depth_stats_host(depth, bitmap, len, pieces, n_pieces, n_long, hist, long_hist, summary, threads); });
}

// The host statement of the pileup SNP model (ug.h) over a flat batch and a
// window (include/fcsug.h): the table, the window's sites (at most max_sites
// are written; the count is returned in *n_sites), and the VCF text of the
// header and of the calls of sites, copied into buf[cap] (the length, or minus the size needed).
int fcsg_ug_table(double pcr_error, int64_t* table) {
  return guard([&] {
    const std::vector<int64_t> t = ug_table(pcr_error);
    std::copy(t.begin(), t.end(), table);
  });
}

int fcsg_ug_sites(const fcsug_batch* b, const fcsug_params* prm, const fcsug_window* w, const uint8_t* ref, const int64_t* table,
                  int threads, fcsug_site* sites, int64_t max_sites, int64_t* n_sites) {
  return guard([&] {
    const std::vector<fcsug_site> s = ug_sites_host(*b, *prm, *w, ref, table, threads);
    if ((int64_t)s.size() > max_sites) throw failedCommand("[E::ug] the window has " + std::to_string(s.size()) + " sites, max_sites is " + std::to_string(max_sites));
    std::copy(s.begin(), s.end(), sites);
    *n_sites = (int64_t)s.size();
  });
}

int fcsg_ug_vcf_text(const fcsug_site* sites, int64_t n, const char* chrom, int64_t window_start, double heterozygosity,
                     double stand_call_conf, double max_deletion_fraction, char* buf, int cap) {
  int rc = 0;
  const int g = guard([&] {
    UgGenotypeParams p;
    p.heterozygosity = heterozygosity, p.stand_call_conf = stand_call_conf, p.max_deletion_fraction = max_deletion_fraction;
    std::string out;
    VcfRecord rec;
    for (int64_t k = 0; k < n; ++k)
      if (ug_genotype(sites[k], p, chrom, window_start, rec)) rec.append_line(out);
    rc = copy_out(out, buf, cap);
  });
  return g ? g : rc;
}

int fcsg_ug_vcf_header(const char* sample, const char* names, const int64_t* lengths, char* buf, int cap) {
  int rc = 0;
  const int g = guard([&] {
    std::vector<std::pair<std::string, int64_t>> contigs;
    for (const std::string& name : split_lines(names)) contigs.emplace_back(name, lengths[contigs.size()]);
    rc = copy_out(ug_vcf_header(sample, contigs).to_text(), buf, cap);
  });
  return g ? g : rc;
}

// The host statement of joint genotyping (joint.h) over the arguments of
// fcsjg_genotype (include/fcsjg.h): the tables with the threshold in units, and
// the outputs of a cohort and its sites on `threads` threads.
int fcsg_jg_tables(double heterozygosity, double stand_call_conf, int n_samples, int32_t* S, int32_t* LG, int32_t* LP,
                   int64_t* min_qual) {
  return guard([&] {
    JointParams p;
    p.heterozygosity = heterozygosity, p.stand_call_conf = stand_call_conf;
    const JointTables t = joint_tables(p, n_samples);
    std::copy(t.S.begin(), t.S.end(), S), std::copy(t.LG.begin(), t.LG.end(), LG), std::copy(t.LP.begin(), t.LP.end(), LP);
    *min_qual = t.min_qual;
  });
}

int fcsg_jg_genotype(const fcsjg_cohort* c, const fcsjg_sites* s, const fcsjg_model* m, int threads, const fcsjg_out* out) {
  return guard([&] { joint_genotype_host(*c, *s, *m, threads, *out); });
}

// The host statement of the callers' pileup (pileup.h) over the arguments of
// fcspu_pile (include/fcspu.h), and the reference model's table, which is the
// one the caller hands the device.
int fcsg_pu_pile(const fcspu_batch* batches, int n_batches, const fcspu_params* prm, const fcspu_window* w, const uint8_t* ref,
                 const int32_t* events_in, const fcspu_out* out) {
  return guard([&] { pileup_host(batches, n_batches, *prm, *w, ref, events_in, *out); });
}

int fcsg_pu_op_events(const fcspu_batch* batch, const fcspu_window* w, const char* contig, int32_t* events) {
  return guard([&] { pileup_ops_host(*batch, *w, std::string(contig, (size_t)w->contig_len), events); });
}

int fcspu_table(double* table) {
  return guard([&] { std::memcpy(table, &ref_model().t[0][0], sizeof(double) * 3 * FCSPU_TABLE_ROWS); });
}

// The host statement of indel realignment (indel.h).  fcsg_ir_score is the
// scoring step's oracle over the arguments of fcsir_score (include/fcsir.h).
// fcsg_ir_targets merges n events (ref, start, end) and writes the targets back
// in place; the number kept is returned.  fcsg_ir_left_align moves the indel
// (a, k) of a one-indel alignment at ref[at]; ins_bases (k codes) rotate in
// place; the new a is returned.  fcsg_ir_clean runs clean(bin) with the host
// scores on a bin given as flat arrays: the window [lo, lo + n_ref) of codes,
// n reads (start, duplicate, CIGAR words and codes / qualities by offsets),
// n_known known indels (pos, k, ins, codes by offsets); the updates come back as
// up_read / up_start / up_nm and CIGAR words by up_cigar_off (at most max_cigar
// words), with the consensus count, the alt read count and the pick in info[3].
int fcsg_ir_score(const fcsir_batch* b, int threads, uint32_t* best, int32_t* off) {
  return guard([&] { ir_score_host(*b, threads, best, off); });
}

int fcsg_ir_targets(int32_t* ref, int64_t* start, int64_t* end, int n) {
  int kept = 0;
  const int g = guard([&] {
    std::vector<IrInterval> ev;
    for (int k = 0; k < n; ++k) ev.push_back({ref[k], start[k], end[k]});
    const std::vector<IrInterval> t = ir_merge_targets(std::move(ev));
    for (size_t k = 0; k < t.size(); ++k) ref[k] = t[k].ref, start[k] = t[k].start, end[k] = t[k].end;
    kept = (int)t.size();
  });
  return g ? g : kept;
}

int fcsg_ir_cigar_events(int32_t ref, int64_t pos, const uint32_t* cigar, int n_cigar, int64_t* start, int64_t* end, int cap) {
  int n = 0;
  const int g = guard([&] {
    std::vector<IrInterval> ev;
    ir_cigar_events(ref, pos, std::vector<uint32_t>(cigar, cigar + n_cigar), ev);
    if ((int)ev.size() > cap) throw failedCommand("[E::indel] more events than the caller has room for");
    for (size_t k = 0; k < ev.size(); ++k) start[k] = ev[k].start, end[k] = ev[k].end;
    n = (int)ev.size();
  });
  return g ? g : n;
}

int fcsg_ir_left_align(const uint8_t* ref, int64_t at, int a, int k, int ins, uint8_t* ins_bases) {
  int out = 0;
  const int g = guard([&] {
    IrIndel d;
    d.a = a, d.k = k, d.ins = ins != 0;
    if (d.ins) d.bases.assign(ins_bases, ins_bases + k);
    ir_left_align(ref, at, d);
    if (d.ins) std::copy(d.bases.begin(), d.bases.end(), ins_bases);
    out = d.a;
  });
  return g ? g : out;
}

int fcsg_ir_clean(int64_t lo, const uint8_t* ref, int64_t n_ref, int n, const int64_t* start, const uint8_t* duplicate,
                  const uint32_t* cigar, const int64_t* cigar_off, const uint8_t* codes, const uint8_t* quals, const int64_t* base_off,
                  int n_known, const int64_t* known_pos, const int32_t* known_k, const uint8_t* known_ins, const uint8_t* known_codes,
                  const int64_t* known_off, int max_reads, int max_consensuses, int lod_tenths, int32_t* up_read, int64_t* up_start,
                  int32_t* up_nm, uint32_t* up_cigar, int64_t* up_cigar_off, int64_t max_cigar, int64_t* info) {
  int n_up = 0;
  const int g = guard([&] {
    IrBin bin;
    bin.lo = lo, bin.hi = lo + n_ref, bin.ref.assign(ref, ref + n_ref);
    for (int i = 0; i < n; ++i) {
      IrRead r;
      r.start = start[i], r.duplicate = duplicate[i] != 0;
      r.cigar.assign(cigar + cigar_off[i], cigar + cigar_off[i + 1]);
      r.codes.assign(codes + base_off[i], codes + base_off[i + 1]), r.quals.assign(quals + base_off[i], quals + base_off[i + 1]);
      bin.reads.push_back(std::move(r));
    }
    for (int i = 0; i < n_known; ++i) {
      IrKnown kn;
      kn.pos = known_pos[i], kn.indel.k = known_k[i], kn.indel.ins = known_ins[i] != 0;
      kn.indel.bases.assign(known_codes + known_off[i], known_codes + known_off[i + 1]);
      bin.known.push_back(std::move(kn));
    }
    IrParams prm;
    prm.max_reads = max_reads, prm.max_consensuses = max_consensuses, prm.lod_tenths = lod_tenths;
    const IrPlan plan = ir_prepare(bin, prm);
    info[0] = (int64_t)plan.cons.size(), info[1] = (int64_t)plan.alt.size(), info[2] = plan.skip;
    std::vector<IrUpdate> ups;
    if (!plan.skip && !plan.cons.empty() && !plan.alt.empty()) {
      IrBatch batch;
      batch.add(bin, plan);
      std::vector<uint32_t> best((size_t)batch.pairs());
      std::vector<int32_t> off((size_t)batch.pairs());
      ir_score_host(batch.view(), 1, best.data(), off.data());
      ups = ir_decide(bin, plan, prm, best.data(), off.data());
    }
    up_cigar_off[0] = 0;
    for (size_t k = 0; k < ups.size(); ++k) {
      up_read[k] = ups[k].read, up_start[k] = ups[k].start, up_nm[k] = ups[k].nm;
      if (up_cigar_off[k] + (int64_t)ups[k].cigar.size() > max_cigar) throw failedCommand("[E::indel] more CIGAR words than the caller has room for");
      std::copy(ups[k].cigar.begin(), ups[k].cigar.end(), up_cigar + up_cigar_off[k]);
      up_cigar_off[k + 1] = up_cigar_off[k] + (int64_t)ups[k].cigar.size();
    }
    n_up = (int)ups.size();
  });
  return g ? g : n_up;
}

int fcsg_bam_index(const char* bam) {
  return guard([&] { bam_index_build(bam); });
}

int fcsg_bam_seek_offset(const char* bai, int tid, long long beg, unsigned long long* off) {
  return guard([&] { *off = BamIndex(bai).seek_offset(tid, beg); });
}

int fcsg_vcf_concat(const char* const* inputs, int n, const char* output) {
  return guard([&] { vcf_concat(std::vector<std::string>(inputs, inputs + n), output); });
}

int fcsg_vcf_concat_bgzip_tabix(const char* const* inputs, int n, const char* plain, const char* gz) {
  return guard([&] { vcf_concat_bgzip_tabix(std::vector<std::string>(inputs, inputs + n), plain, gz); });
}

int fcsg_bgzip_tabix(const char* in, const char* out) {
  return guard([&] { bgzip_tabix_file(in, out); });
}
int fcsg_tabix(const char* vcf_gz) {
  return guard([&] { tabix_index_vcf(vcf_gz); });
}

unsigned fcsg_reg2bin(long long beg, long long end) { return reg2bin(beg, end); }

// Runs an executor with n_tasks shell-command workers (cmd per task, %d = task
// index) over n_threads threads and GPU slots gpus_csv; writes the per-task
// FCS_GPU_DEVICE seen by each command into its own output.  Returns the
// exception class on failure: 0 ok, 4 failedCommand, 1 other; findError text in buf.
int fcsg_run_stage(const char* cmd_fmt, int n_tasks, int n_threads, const char* gpus_csv, const char* log_dir,
                   char* buf, int cap) {
  try {
    conf().init("");
    conf().set("log_dir", log_dir);
    std::vector<int> gpus;
    std::string g = gpus_csv;
    for (size_t p = 0; p < g.size();) {
      const size_t e = std::min(g.find(',', p), g.size());
      if (e > p) gpus.push_back(std::stoi(g.substr(p, e - p)));
      p = e + 1;
    }
    class Cmd : public Worker {
     public:
      explicit Cmd(std::string c) : Worker(1, 1, {}, "test stage") { cmd_ = std::move(c); }
    };
    Executor ex("test", n_threads, gpus);
    for (int i = 0; i < n_tasks; ++i) {
      char c[4096];
      std::snprintf(c, sizeof c, cmd_fmt, i);
      ex.addTask(std::make_shared<Cmd>(c), "");
    }
    ex.run();
    copy_out("", buf, cap);
    return 0;
  } catch (const failedCommand&) {
    copy_out(g_err, buf, cap);
    return 4;
  } catch (const std::exception& e) {
    g_err = e.what();
    copy_out(g_err, buf, cap);
    return 1;
  }
}

int fcsg_find_error(const char* const* logs, int n, char* buf, int cap) {
  return copy_out(LogUtils::findError(std::vector<std::string>(logs, logs + n)), buf, cap);
}

// The host statement of minimizer seeding and chaining (minimizer.h).
// fcsg_mm_sketch writes the minimizers of n codes (hash, position of the last
// base, strand) and returns their number.  fcsg_mm_anchors builds the index of
// n_contigs contigs (codes by offsets) and writes one read's anchors and
// frac_rep.  fcsg_mm_chain is the recurrence's oracle over the arguments of
// fcsmm_chain (include/fcsmm.h).  fcsg_mm_backtrack writes the kept chains of
// one read: score[c] and the anchors anchors[chain_off[c] .. chain_off[c + 1]).
// A count above cap is an error.
int fcsg_mm_sketch(const uint8_t* codes, int64_t n, int k, int w, uint64_t* h, int32_t* pos, uint8_t* strand, int cap) {
  int count = 0;
  const int g = guard([&] {
    std::vector<MmMini> m;
    mm_sketch(codes, n, k, w, m);
    if ((int64_t)m.size() > cap) throw invalidParam("fcsg_mm_sketch: more minimizers than cap");
    for (size_t i = 0; i < m.size(); ++i) h[i] = m[i].h, pos[i] = m[i].pos, strand[i] = m[i].strand;
    count = (int)m.size();
  });
  return g ? g : count;
}

int fcsg_mm_anchors(const uint8_t* ref, const int64_t* ref_off, int n_contigs, const uint8_t* read, int L, int k, int w, int max_occ,
                    int64_t* t, int32_t* q, int cap, double* frac_rep) {
  int count = 0;
  const int g = guard([&] {
    std::vector<std::vector<uint8_t>> contigs;
    for (int c = 0; c < n_contigs; ++c) contigs.emplace_back(ref + ref_off[c], ref + ref_off[c + 1]);
    const MmIndex idx(contigs, k, w);
    std::vector<int64_t> tv;
    std::vector<int32_t> qv;
    mm_read_anchors(idx, read, L, max_occ, tv, qv, *frac_rep);
    if ((int64_t)tv.size() > cap) throw invalidParam("fcsg_mm_anchors: more anchors than cap");
    std::copy(tv.begin(), tv.end(), t), std::copy(qv.begin(), qv.end(), q);
    count = (int)tv.size();
  });
  return g ? g : count;
}

int fcsg_mm_chain(const fcsmm_batch* b, int threads, int32_t* f, int32_t* p) {
  return guard([&] { mm_chain_host(*b, threads, f, p); });
}

int fcsg_mm_backtrack(const int32_t* f, const int32_t* p, int n, int min_cnt, int min_score, int32_t* score, int32_t* chain_off,
                      int32_t* anchors, int cap) {
  int count = 0;
  const int g = guard([&] {
    std::vector<MmChain> ch;
    mm_backtrack(f, p, n, min_cnt, min_score, ch);
    if ((int64_t)ch.size() > cap) throw invalidParam("fcsg_mm_backtrack: more chains than cap");
    int32_t at = 0;
    for (size_t c = 0; c < ch.size(); ++c) {
      score[c] = ch[c].score, chain_off[c] = at;
      for (int32_t a : ch[c].anchors) anchors[at++] = a;
    }
    chain_off[ch.size()] = at;
    count = (int)ch.size();
  });
  return g ? g : count;
}

}  // extern "C"
