// The ug command (ug_run.h): the BAM streams in chunks of ug.chunk_records;
// the genome is walked in windows of at most ug.window_bp loci over the
// contigs that hold intervals; the records that overlap a window are gathered
// until the stream has passed its end, piled up in one call and genotyped; a
// record is given to every window it overlaps.
#include "ug_run.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "bam.h"
#include "common.h"
#include "config.h"
#include "depth_run.h"
#include "fasta.h"
#include "fcship.h"
#include "flat_batch.h"
#include "ug.h"
#include "vcf.h"

namespace fcsg {

namespace {

struct UgApi {
  decltype(&fcsug_sites) sites = FCSG_DEVICE_ENTRY(fcsug_sites);
  LastErrorFn last_error = last_error_entry();
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

struct Part {
  int64_t start, end;  // window offsets
};

struct Window {
  fcsug_window w;
  std::vector<Part> parts;
};

// The sort key of a record: unmapped records without a contig come last.
std::pair<int64_t, int64_t> key_of(int32_t ref_id, int32_t pos) { return {ref_id < 0 ? (int64_t)INT32_MAX + 1 : ref_id, pos}; }

class Run {
 public:
  explicit Run(const UgJob& job)
      : job_(job),
        device_(device_or_host(job.device, gpu_ug_available(),
                               "[fcs-genome ug] ug.gpu: the loaded libfcship has no fcsug_sites entry point; "
                               "sites are piled up on the host\n")),
        bams_(sorted_bam_inputs(job.input)) {
    reader_.reset(new BamReader(bams_[0]));
    header_ = reader_->header();
    st_.sample = single_sample(header_, "ug");
    const Reference ref = load_fasta(job.ref);
    contigs_.resize(header_.names.size());
    for (size_t k = 0; k < header_.names.size(); ++k) {
      const int c = ref.index(header_.names[k]);
      if (c < 0) throw invalidParam("contig " + header_.names[k] + " of the BAM header is not in " + job.ref);
      contigs_[k] = ref.contigs[(size_t)c].seq;
      if ((int64_t)contigs_[k].size() != header_.lengths[k])
        throw invalidParam("contig " + header_.names[k] + " has " + std::to_string(header_.lengths[k]) +
                           " bases in the BAM header and " + std::to_string(contigs_[k].size()) + " in " + job.ref);
    }
    Config& cf = conf();
    prm_.min_baseq = cf.get_int("ug.min_baseq");
    geno_.stand_call_conf = conf_double("ug.stand_call_conf");
    geno_.heterozygosity = conf_double("ug.heterozygosity");
    geno_.max_deletion_fraction = conf_double("ug.max_deletion_fraction");
    if (!(geno_.heterozygosity > 0.0 && geno_.heterozygosity < 2.0 / 3.0))
      throw invalidParam("ug.heterozygosity " + std::to_string(geno_.heterozygosity) + " is outside (0, 2/3)");
    table_ = ug_table(conf_double("ug.pcr_error"));
    chunk_ = (size_t)std::max(cf.get_int("ug.chunk_records"), 1);
    window_bp_ = std::clamp<int64_t>(cf.get_int("ug.window_bp"), 1, FCSUG_WINDOW_MAX);
    intervals_ = merged_intervals(job.intervals, header_);
    cut_windows();
  }

  UgRunStats run() {
    const uint64_t t0 = now_us();
    try {
      std::vector<std::pair<std::string, int64_t>> contigs;
      for (size_t k = 0; k < header_.names.size(); ++k) contigs.emplace_back(header_.names[k], header_.lengths[k]);
      VcfWriter out(job_.output, ug_vcf_header(st_.sample, contigs));
      FlatRecords f;
      for (const Window& win : windows_) {
        call_window(win, f, out);
        if (interrupted()) throw interruptedError();
      }
      while (!eof_) buf_.clear(), read_chunk();  // the rest of the stream is still checked for its order
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
  // Windows of at most window_bp loci from each contig's first interval start to its last interval end.
  void cut_windows() {
    for (size_t a = 0; a < intervals_.size();) {
      size_t b = a;
      while (b < intervals_.size() && intervals_[b].ref == intervals_[a].ref) ++b;
      const int32_t ref = intervals_[a].ref;
      size_t k = a;
      for (int64_t s = intervals_[a].start; s < intervals_[b - 1].end; s += window_bp_) {
        Window win;
        win.w.ref_id = ref, win.w.reserved = 0, win.w.start = s;
        win.w.len = std::min(window_bp_, intervals_[b - 1].end - s), win.w.contig_len = header_.lengths[(size_t)ref];
        const int64_t e = s + win.w.len;
        while (k < b && intervals_[k].end <= s) ++k;
        for (size_t j = k; j < b && intervals_[j].start < e; ++j)
          win.parts.push_back({std::max(intervals_[j].start, s) - s, std::min(intervals_[j].end, e) - s});
        if (!win.parts.empty()) windows_.push_back(std::move(win));
      }
      a = b;
    }
  }

  // Up to chunk_ more records at the end of buf_.
  void read_chunk() {
    BamRecord r;
    for (size_t got = 0; got < chunk_;) {
      if (!reader_->next(r)) {
        if (++file_ >= bams_.size()) {
          eof_ = true;
          break;
        }
        reader_.reset(new BamReader(bams_[file_]));
        continue;
      }
      const auto key = key_of(r.ref_id, r.pos);
      if (key < last_key_) {
        auto where = [&](int64_t ref, int64_t pos) {
          return (ref >= 0 && ref < (int64_t)header_.names.size() ? header_.names[(size_t)ref] : std::string("*")) + ":" +
                 std::to_string(pos + 1);
        };
        throw invalidParam("the input is not coordinate-sorted: record " + r.name + " at " + where(r.ref_id, r.pos) +
                           " follows one at " + where(last_key_.first, last_key_.second));
      }
      last_key_ = key;
      buf_.push_back(std::move(r));
      ++got, ++st_.records;
    }
  }

  void call_window(const Window& win, FlatRecords& f, VcfWriter& out) {
    const fcsug_window& w = win.w;
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
    while (!eof_ && (buf_.empty() || key_of(buf_.back().ref_id, buf_.back().pos) < past)) read_chunk(), drop();
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
      if (ug_api().sites(device_, &view, &prm_, &w, ref, table_.data(), room_.get(), w.len, &found) != FCS_OK)
        throw failedCommand(std::string("[E::fcs-genome ug] fcsug_sites: ") + ug_api().last_error());
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
  std::vector<std::string> bams_;
  std::unique_ptr<BamReader> reader_;
  size_t file_ = 0, chunk_ = 1;
  bool eof_ = false;
  BamHeader header_;
  std::vector<std::string> contigs_;
  fcsug_params prm_{};
  UgGenotypeParams geno_;
  std::vector<int64_t> table_;
  int64_t window_bp_ = 1;
  std::vector<GenomeInterval> intervals_;
  std::vector<Window> windows_;
  std::vector<BamRecord> buf_;
  std::unique_ptr<fcsug_site[]> room_;  // the device call's sites, one window's worth
  int64_t room_len_ = 0;
  std::pair<int64_t, int64_t> last_key_{-1, -1};
  UgRunStats st_;
};

}  // namespace

bool gpu_ug_available() {
  const UgApi& a = ug_api();
  return a.sites && a.last_error;
}

std::vector<std::string> ug_output_files(const UgJob& job) {
  return {job.output, job.output + ".gz", job.output + ".gz.tbi"};
}

UgRunStats ug_run(const UgJob& job) { return Run(job).run(); }

}  // namespace fcsg
