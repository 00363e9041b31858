// The ug command (ug_run.h): the BAM streams in chunks of ug.chunk_records;
// the genome is walked in windows of at most ug.window_bp loci over the
// contigs that hold intervals; the records that overlap a window are gathered
// until the stream has passed its end, piled up in one call and genotyped; a
// record is given to every window it overlaps.
#include "ug_run.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "bam_stream.h"
#include "common.h"
#include "config.h"
#include "fcship.h"
#include "flat_batch.h"
#include "ug.h"
#include "vcf.h"

namespace fcsg {

namespace {

struct UgApi {
  decltype(&fcsug_sites) sites = FCSG_DEVICE_ENTRY(fcsug_sites);
};

const UgApi& ug_api() {
  static const UgApi A;
  return A;
}

// A configuration key that holds a number.
double conf_double(const std::string& key) {
  const std::string v = conf().get_string(key);
  char* end = nullptr;
  const double d = std::strtod(v.c_str(), &end);
  if (v.empty() || *end) throw invalidParam(key + " = " + v + " is not a number");
  return d;
}

class Run {
 public:
  explicit Run(const UgJob& job)
      : job_(job),
        device_(device_or_host(job.device, gpu_ug_available(),
                               "[fcs-genome ug] ug.gpu: the loaded libfcship has no fcsug_sites entry point; "
                               "sites are piled up on the host\n")),
        in_(job.input, true),
        header_(in_.header()) {
    st_.sample = single_sample(header_, "ug");
    contigs_ = header_contigs(job.ref, header_, true);
    Config& cf = conf();
    prm_.min_baseq = cf.get_int("ug.min_baseq");
    geno_.stand_call_conf = conf_double("ug.stand_call_conf");
    geno_.heterozygosity = conf_double("ug.heterozygosity");
    geno_.max_deletion_fraction = conf_double("ug.max_deletion_fraction");
    if (!(geno_.heterozygosity > 0.0 && geno_.heterozygosity < 2.0 / 3.0))
      throw invalidParam("ug.heterozygosity " + std::to_string(geno_.heterozygosity) + " is outside (0, 2/3)");
    table_ = ug_table(conf_double("ug.pcr_error"));
    chunk_ = (size_t)std::max(cf.get_int("ug.chunk_records"), 1);
    const int64_t window_bp = std::clamp<int64_t>(cf.get_int("ug.window_bp"), 1, FCSUG_WINDOW_MAX);
    intervals_ = merged_intervals(job.intervals, header_);
    windows_ = cut_windows(intervals_, header_.lengths, window_bp);
  }

  UgRunStats run() {
    const uint64_t t0 = now_us();
    try {
      std::vector<std::pair<std::string, int64_t>> contigs;
      for (size_t k = 0; k < header_.names.size(); ++k) contigs.emplace_back(header_.names[k], header_.lengths[k]);
      VcfWriter out(job_.output, ug_vcf_header(st_.sample, contigs));
      FlatRecords f;
      for (const GenomeWindow& win : windows_) {
        call_window(win, f, out);
        if (interrupted()) throw interruptedError();
      }
      while (!in_.eof()) buf_.clear(), read_chunk();  // the rest of the stream is still checked for its order
      out.close();
      bgzip_tabix_file(job_.output, job_.output + ".gz");
    } catch (...) {  // a refused run leaves no partial file
      for (const std::string& f : ug_output_files(job_)) remove_path(f);
      throw;
    }
    st_.windows = (int64_t)windows_.size(), st_.intervals = (int64_t)intervals_.size();
    st_.on_device = device_ >= 0;
    st_.seconds = (now_us() - t0) / 1e6;
    return st_;
  }

 private:
  // Up to chunk_ more records at the end of buf_.
  void read_chunk() { st_.records += (int64_t)in_.read(buf_, chunk_); }

  void call_window(const GenomeWindow& win, FlatRecords& f, VcfWriter& out) {
    const fcsug_window w = win.as<fcsug_window>();
    const std::pair<int64_t, int64_t> past{w.ref_id, w.start + w.len};
    // records the stream has left behind: earlier contigs, and those that end before the window's start
    auto drop = [&] {
      buf_.erase(std::remove_if(buf_.begin(), buf_.end(),
                                [&](const BamRecord& r) {
                                  return r.ref_id >= 0 && (r.ref_id < w.ref_id || (r.ref_id == w.ref_id && r.pos < w.start &&
                                                                                   r.end() <= w.start));
                                }),
                 buf_.end());
    };
    drop();
    while (!in_.eof() && (buf_.empty() || key_of(buf_.back().ref_id, buf_.back().pos) < past)) read_chunk(), drop();
    size_t n = 0;
    while (n < buf_.size() && key_of(buf_[n].ref_id, buf_[n].pos) < past) ++n;
    if (n == 0) return;
    flatten(buf_, n, true, f);
    const fcsug_batch view = f.view<fcsug_batch>(0, n);
    const uint8_t* ref = reinterpret_cast<const uint8_t*>(contigs_[(size_t)w.ref_id].data()) + w.start;
    std::vector<fcsug_site> host_sites;
    const fcsug_site* sites = nullptr;
    int64_t found = 0;
    if (device_ >= 0) {
      if (room_len_ < w.len) room_.reset(new fcsug_site[(size_t)w.len]), room_len_ = w.len;  // not zeroed: only [0, found) is read
      device_check(ug_api().sites(device_, &view, &prm_, &w, ref, table_.data(), room_.get(), w.len, &found), "ug", "fcsug_sites");
      sites = room_.get();
    } else {
      host_sites = ug_sites_host(view, prm_, w, ref, table_.data(), host_threads());
      sites = host_sites.data(), found = (int64_t)host_sites.size();
    }
    st_.sites += found;
    VcfRecord rec;
    size_t part = 0;
    const std::string& chrom = header_.names[(size_t)w.ref_id];
    for (int64_t k = 0; k < found; ++k) {
      const fcsug_site& s = sites[k];
      while (part < win.parts.size() && win.parts[part].end <= s.offset) ++part;
      if (part == win.parts.size()) break;
      if (s.offset < win.parts[part].start) continue;  // outside the intervals
      if (!ug_genotype(s, geno_, chrom, w.start, rec)) continue;
      out.write(rec);
      ++st_.calls;
    }
  }

  const UgJob& job_;
  int device_;
  BamStream in_;
  const BamHeader& header_;
  size_t chunk_ = 1;
  std::vector<std::string> contigs_;
  fcsug_params prm_{};
  UgGenotypeParams geno_;
  std::vector<int64_t> table_;
  std::vector<GenomeInterval> intervals_;
  std::vector<GenomeWindow> windows_;
  std::vector<BamRecord> buf_;
  std::unique_ptr<fcsug_site[]> room_;  // the device call's sites, one window's worth
  int64_t room_len_ = 0;
  UgRunStats st_;
};

}  // namespace

bool gpu_ug_available() {
  const UgApi& a = ug_api();
  return a.sites && last_error_entry();
}

std::vector<std::string> ug_output_files(const UgJob& job) {
  return {job.output, job.output + ".gz", job.output + ".gz.tbi"};
}

UgRunStats ug_run(const UgJob& job) { return Run(job).run(); }

}  // namespace fcsg
