// fcs-genome command line: the reference's CLI surface
// for the GPU-backed commands — `htc`, `mutect2`, `align` — with its option
// names (src/worker-htc.cpp:25-33, src/worker-mutect2.cpp:26-40,
// src/worker-align.cpp:29-42), config keys (`conf`) and exit codes
// (src/main.cpp:165-240: help 0, bad option 1/2, missing file 3, failed
// stage 4, other error -1), plus `synth` for the synthetic C1/C4/C5 inputs.
#include <algorithm>
#include <malloc.h>
#include <sys/resource.h>
#include <unistd.h>

#include <cerrno>

#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <thread>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "config.h"
#include "executor.h"
#include "fcship.h"
#include "aligner.h"
#include "bqsr_run.h"
#include "depth_run.h"
#include "indel_run.h"
#include "joint_run.h"
#include "ug_run.h"
#include "intervals.h"
#include "markdup.h"
#include "sample_sheet.h"
#include "synth.h"
#include "workers.h"

namespace fcsg {

namespace {

// Minimal boost::program_options stand-in: long/short options with values or flags.
class Args {
 public:
  struct Opt {
    std::string lng, shrt, help;
    bool flag, required;
  };
  void add(const std::string& lng, const std::string& shrt, bool flag, bool required, const std::string& help) {
    opts_.push_back({lng, shrt, help, flag, required});
  }
  void parse(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
      std::string a = argv[i];
      if (a == "-h" || a == "--help") throw helpRequest();
      const Opt* o = nullptr;
      std::string val;
      bool has_val = false;
      for (const Opt& x : opts_) {
        if (a == "--" + x.lng || (!x.shrt.empty() && a == "-" + x.shrt)) o = &x;
        else if (a.rfind("--" + x.lng + "=", 0) == 0) {
          o = &x;
          val = a.substr(x.lng.size() + 3);
          has_val = true;
        }
        if (o) break;
      }
      if (!o) throw invalidParam(a);
      if (o->flag) {
        vals_[o->lng].push_back("1");
        continue;
      }
      if (!has_val) {
        if (i + 1 >= argc) throw invalidParam(a + " needs a value");
        val = argv[++i];
      }
      vals_[o->lng].push_back(val);
    }
    for (const Opt& x : opts_)
      if (x.required && !vals_.count(x.lng)) throw invalidParam("--" + x.lng + " is required");
  }
  bool has(const std::string& k) const { return vals_.count(k) > 0; }
  std::string get(const std::string& k, const std::string& def = "") const {
    auto it = vals_.find(k);
    if (it == vals_.end()) return def;
    if (it->second.back().empty()) throw pathEmpty(k);
    return it->second.back();
  }
  std::vector<std::string> all(const std::string& k) const {
    auto it = vals_.find(k);
    return it == vals_.end() ? std::vector<std::string>{} : it->second;
  }
  std::string help() const {
    std::string s;
    for (const Opt& x : opts_)
      s += "  " + (x.shrt.empty() ? std::string("    ") : "-" + x.shrt + ", ") + "--" + x.lng +
           (x.flag ? "" : " arg") + "\t" + x.help + "\n";
    return s;
  }

 private:
  std::vector<Opt> opts_;
  std::map<std::string, std::vector<std::string>> vals_;
};

void common_opts(Args& a) {
  a.add("force", "f", true, false, "overwrite output files if they exist");
  a.add("extra-options", "O", false, false, "extra options for the command");
}

std::vector<int> slots() {
  std::vector<int> g = conf().gpu_devices();
  if (g.empty()) throw failedCommand("[E::fcs-genome] no GPU visible (gpu.devices); the GPU path has no CPU fallback");
  return g;
}

// gpu.bgzf_deflate: the device the final VCF.gz's blocks compress on (the first slot's), or -1.
int bgzf_device(const std::vector<int>& gpus) {
  if (!conf().get_bool("gpu.bgzf_deflate")) return -1;
  for (int d : gpus)
    if (d >= 0) return d;
  return -1;
}

// Shards of the run: -L list (one file for all shards) or the reference's 32 interval parts.
std::vector<std::vector<std::string>> shard_intervals(const std::string& ref, const std::string& intv_list) {
  const int n = conf().get_int("gatk.ncontigs");
  std::vector<std::vector<std::string>> out(n);
  if (!intv_list.empty()) {
    // split the user's list into n shard files, contig order preserved
    const auto iv = read_interval_list(intv_list);
    std::vector<std::pair<std::string, int64_t>> pseudo;  // (name, length) of each listed interval
    for (const Interval& i : iv) pseudo.emplace_back(i.chrom, i.ub - i.lb + 1);
    const auto parts = partition_contigs(pseudo, n, false);
    const std::string dir = conf().temp_dir() + "/intv_user";
    create_dir(dir);
    for (int k = 0; k < n; ++k) {
      std::vector<Interval> shifted;
      for (const Interval& p : parts[k]) {
        // map back: pseudo-contig i starts at iv[i].lb
        for (const Interval& src : iv)
          if (src.chrom == p.chrom && p.lb - 1 + src.lb <= src.ub) {
            shifted.push_back({src.chrom, src.lb + p.lb - 1, src.lb + p.ub - 1});
            break;
          }
      }
      const std::string path = get_contig_fname(dir, k, "list", "part-");
      write_interval_list(path, shifted);
      out[k].push_back(path);
    }
    return out;
  }
  const auto paths = init_contig_intv(ref, n, conf().temp_dir(), conf().get_bool("gatk.skip_pseudo_chr"));
  for (int k = 0; k < n; ++k) out[k].push_back(paths[k]);
  return out;
}

// Shards of a directory input (BamInput): the parts' region files give the
// intervals, so only the user's -L (if any) goes to every shard
// (src/worker-htc.cpp:88-97: init_contig_intv only for a regular-file input).
std::vector<std::vector<std::string>> dir_shards(const std::string& intv_list) {
  std::vector<std::vector<std::string>> out(conf().get_int("gatk.ncontigs"));
  if (!intv_list.empty())
    for (auto& v : out) v.push_back(intv_list);
  return out;
}

// FCS_TIMELINE=1: seconds since the process started at named points
// (where a command's wall time goes outside its stages)
void timeline(const char* what) {
  static const bool on = [] {
    const char* e = std::getenv("FCS_TIMELINE");
    return e && *e && *e != '0';
  }();
  if (!on) return;
  double up = 0, start = 0;
  if (std::FILE* f = std::fopen("/proc/uptime", "r")) {
    if (std::fscanf(f, "%lf", &up) != 1) up = 0;
    std::fclose(f);
  }
  if (std::FILE* f = std::fopen("/proc/self/stat", "r")) {
    char buf[1024];
    const size_t n = std::fread(buf, 1, sizeof buf - 1, f);
    std::fclose(f);
    buf[n] = 0;
    const char* p = std::strrchr(buf, ')');  // fields after the command name; starttime is field 22
    unsigned long long ticks = 0;
    for (int field = 3; p && *p && field <= 22; ++field) {
      p = std::strchr(p + 1, ' ');
      if (p && field == 22) ticks = std::strtoull(p + 1, nullptr, 10);
    }
    start = (double)ticks / (double)sysconf(_SC_CLK_TCK);
  }
  struct rusage ru {};
  getrusage(RUSAGE_SELF, &ru);
  char line[256];
  std::snprintf(line, sizeof line, "[fcs-genome timeline] %s %.2f s (user %.2f s, sys %.2f s, minor faults %ld, csw %ld/%ld)",
                what, up - start, ru.ru_utime.tv_sec + ru.ru_utime.tv_usec / 1e6,
                ru.ru_stime.tv_sec + ru.ru_stime.tv_usec / 1e6, ru.ru_minflt, ru.ru_nvcsw, ru.ru_nivcsw);
  std::cerr << line << std::endl;
}

// What `htc` queues over one BAM (or directory of part BAMs): the shard tasks,
// the concat to <output> + .gz + .tbi, and the warm-up and release workers.
// `germline` runs the same stages over the BAM it aligned.
struct HtcRun {
  std::string ref, input, output, intervals, sample_id;
  std::vector<std::string> extra;
  bool force = false, produce_vcf = false, skip_concat = false;
};

void run_htc(const HtcRun& r, const std::vector<int>& gpus) {
  const std::string &ref = r.ref, &input = r.input, &output = r.output, &sample_id = r.sample_id;
  const std::vector<std::string>& extra = r.extra;
  const bool force = r.force;
  const std::string out_dir = conf().temp_dir() + "/htc";
  create_dir(out_dir);
  const bool flag_vcf = r.produce_vcf;
  const auto shards = is_directory(input) ? dir_shards(r.intervals) : shard_intervals(ref, r.intervals);
  timeline("shards");
  // the GPU runtime and tables come up in the background while the first
  // shards decode and pile up their reads (the reference's BackgroundExecutor
  // NAM daemon runs beside its Executor the same way)
  BackgroundExecutor warm("gpu-warmup", std::make_shared<DeviceWarmupWorker>(gpus));
  Executor ex("Haplotype Caller", conf().get_int("gatk.htc.nprocs", "gatk.nprocs"), gpus);
  std::vector<std::string> parts;
  for (size_t k = 0; k < shards.size(); ++k) {
    const std::string part = get_contig_fname(out_dir, (int)k, flag_vcf ? "vcf" : "g.vcf");
    parts.push_back(part);
    ex.addTask(std::make_shared<HTCWorker>(ref, shards[k], input, part, extra, (int)k, flag_vcf, true), sample_id);
  }
  const std::string plain = output;
  if (!r.skip_concat) {
    if (!force && path_exists(plain + ".gz")) throw invalidParam("output " + plain + ".gz exists (use -f)");
    // concat -> bgzip -> tabix as one pass over the parts
    ex.addTask(std::make_shared<VCFConcatWorker>(parts, plain, plain + ".gz", /*consume=*/true, bgzf_device(gpus)),
               sample_id, true);
  } else {
    ex.addTask(std::make_shared<VCFConcatWorker>(parts, plain), sample_id, true);
  }
  // with gpu.bgzf_deflate the tail compresses on a device: the release waits for it (a stage of its own)
  if (conf().get_bool("gpu.release_early"))
    ex.addTask(std::make_shared<GpuReleaseWorker>(gpus, &warm), sample_id, bgzf_device(gpus) >= 0);
  timeline("stages queued");
  ex.run();
  timeline("stages done");
  warm.wait();
  timeline("warm-up joined");
  if (warm.status() != 0) throw failedCommand(std::string("[E::fcs-genome] GPU warm-up failed: ") + fcs_last_error());
}

int htc_main(int argc, char** argv) {
  Args a;
  common_opts(a);
  a.add("ref", "r", false, true, "reference genome path");
  a.add("input", "i", false, true, "input BAM file or directory of part-XXXXXX.bam + .bed/.list");
  a.add("output", "o", false, true, "output GVCF/VCF file (<output>.gz + .tbi are written too)");
  a.add("produce-vcf", "v", true, false, "produce VCF instead of GVCF (reference-confidence blocks)");
  a.add("intervalList", "L", false, false, "interval list file");
  a.add("sample-id", "", false, false, "sample id for log files");
  a.add("skip-concat", "s", true, false, "(deprecated) produce a set of VCF files instead of one");
  a.add("gatk4", "g", true, false, "accepted for compatibility");
  a.add("dump-regions", "", false, false, "debug: write every region's PairHMM inputs/outputs to <path>.<shard>");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome htc' options:\n" << a.help();
    throw;
  }
  HtcRun r;
  r.ref = a.get("ref"), r.input = a.get("input"), r.output = a.get("output"), r.intervals = a.get("intervalList");
  r.sample_id = a.get("sample-id");
  r.extra = a.all("extra-options");
  if (a.has("dump-regions")) r.extra.push_back("--dump-regions " + a.get("dump-regions"));
  r.force = a.has("force"), r.produce_vcf = a.has("produce-vcf"), r.skip_concat = a.has("skip-concat");
  timeline("options parsed");
  run_htc(r, slots());
  return 0;
}

int mutect2_main(int argc, char** argv) {
  Args a;
  common_opts(a);
  a.add("ref", "r", false, true, "reference genome path");
  a.add("normal", "n", false, true, "input normal BAM file or directory");
  a.add("tumor", "t", false, true, "input tumor BAM file or directory");
  a.add("output", "o", false, true, "output VCF file");
  a.add("intervalList", "L", false, false, "interval list file");
  a.add("normal_name", "a", false, false, "normal sample name");
  a.add("tumor_name", "b", false, false, "tumor sample name");
  a.add("sample-id", "", false, false, "sample id for log file");
  for (const char* k : {"dbsnp", "cosmic", "germline", "panels_of_normals", "contamination_table", "filtered_vcf"})
    a.add(k, "", false, false, "accepted for compatibility (not used by the GPU caller)");
  a.add("dump-regions", "", false, false, "debug: write every region's PairHMM inputs/outputs to <path>.<shard>");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome mutect2' options:\n" << a.help();
    throw;
  }
  const std::string ref = a.get("ref"), output = a.get("output");
  const std::vector<int> gpus = slots();
  const std::string out_dir = conf().temp_dir() + "/mutect2";
  create_dir(out_dir);
  // reference intervals only when both inputs are plain BAM files (src/worker-mutect2.cpp:146-150)
  const auto shards = (is_regular_file(a.get("normal")) && is_regular_file(a.get("tumor")))
                          ? shard_intervals(ref, a.get("intervalList"))
                          : dir_shards(a.get("intervalList"));
  BackgroundExecutor warm("gpu-warmup", std::make_shared<DeviceWarmupWorker>(gpus));
  Executor ex("Mutect2", conf().get_int("gatk.mutect2.nprocs", "gatk.nprocs"), gpus);
  std::vector<std::string> parts;
  const std::string sample_id = a.get("sample-id");
  std::vector<std::string> extra = a.all("extra-options");
  if (a.has("dump-regions")) extra.push_back("--dump-regions " + a.get("dump-regions"));
  for (size_t k = 0; k < shards.size(); ++k) {
    const std::string part = get_contig_fname(out_dir, (int)k, "vcf");
    parts.push_back(part);
    ex.addTask(std::make_shared<Mutect2Worker>(ref, shards[k], a.get("normal"), a.get("tumor"), part, extra, (int)k,
                                               true),
               sample_id);
  }
  ex.addTask(std::make_shared<VCFConcatWorker>(parts, output, output + ".gz", /*consume=*/true, bgzf_device(gpus)),
             sample_id, true);
  if (conf().get_bool("gpu.release_early"))
    ex.addTask(std::make_shared<GpuReleaseWorker>(gpus, &warm), sample_id, bgzf_device(gpus) >= 0);
  ex.run();
  warm.wait();
  if (warm.status() != 0) throw failedCommand(std::string("[E::fcs-genome] GPU warm-up failed: ") + fcs_last_error());
  return 0;
}

// One sample of `align` or `germline`: a BWAWorker per read group, each in its
// own stage and on every GPU slot, and a merge stage when there are several.
struct AlignRun {
  std::string ref;
  std::vector<std::string> extra;
  bool force = false, disable_merge = false, align_only = false;
  std::string seeder;      // empty: the key bwa.seeder
  std::string chains_out;  // --chains-out; with a sample sheet .<sample>, with several read groups .<read group> is appended
};

void align_sample(const AlignRun& r, const std::string& sample_id, const std::vector<SampleDetails>& list, const std::string& merged,
                  bool from_sheet, const std::vector<int>& gpus) {
  const std::string temp_dir = conf().temp_dir() + "/align";
  create_dir(temp_dir);
  // one Executor per sample (the reference runs it inside the sample loop);
  // one task at a time, each task on every GPU slot
  Executor ex("align", 1, gpus);
  const std::string merge_dir = temp_dir + "/" + sample_id + "merge";
  create_dir(merge_dir);
  std::vector<std::string> rg_out;
  for (const SampleDetails& d : list) {
    const std::string out_rg = list.size() == 1 ? merged : merge_dir + "/" + sample_id + "_" + d.ReadGroup + ".bam";
    // two read groups of one sample writing one BAM would lose one lane and
    // merge the other twice, silently
    if (std::find(rg_out.begin(), rg_out.end(), out_rg) != rg_out.end())
      throw invalidParam("sample " + sample_id + " lists read group " + d.ReadGroup +
                         " more than once (each read group is aligned to its own BAM)");
    rg_out.push_back(out_rg);
    auto w = std::make_shared<BWAWorker>(r.ref, d.fastqR1, d.fastqR2, out_rg, r.extra, sample_id, d.ReadGroup, d.Platform,
                                         d.LibraryID, !r.disable_merge, r.force || list.size() > 1, gpus, r.align_only);
    std::string chains = r.chains_out;
    if (!chains.empty() && from_sheet) chains += "." + sample_id;
    if (!chains.empty() && list.size() > 1) chains += "." + d.ReadGroup;
    w->set_seeding(r.seeder, chains);
    ex.addTask(w, sample_id, true);
  }
  if (list.size() > 1) {
    if (!r.disable_merge) {
      ex.addTask(std::make_shared<MergeBamWorker>(rg_out, merged, r.force), sample_id, true);
    } else {  // bucket i of every read group -> bucket i of the sample (worker-align.cpp:226-246)
      create_dir(merged);
      const int nb = std::max(1, conf().get_int("bwa.num_buckets"));
      for (int i = 0; i < nb; ++i) {
        std::vector<std::string> in;
        for (const std::string& rg : rg_out) in.push_back(get_contig_fname(rg, i, "bam"));
        ex.addTask(std::make_shared<MergeBamWorker>(in, get_contig_fname(merged, i, "bam"), true), sample_id, i == 0);
      }
    }
  }
  ex.run();
}

// `fcs-genome align` (reference src/worker-align.cpp:19-256): a single read
// group (-1/-2, -R/-S/-P/-L) or a sample sheet (-F; file or FASTQ folder).
// One BWAWorker per (sample, read group), each in its own stage and on every
// GPU slot; a sample with several read groups gets a merge stage.  The
// reference's sambamba INDEX stage is not needed: BAMs are written with their
// index.  Without -F a single-end run (-1 only) is accepted as well.
int align_main(int argc, char** argv) {
  Args a;
  common_opts(a);
  a.add("ref", "r", false, true, "reference genome path");
  a.add("fastq1", "1", false, false, "input pair-end fastq file (plain or .gz)");
  a.add("fastq2", "2", false, false, "input pair-end fastq file (plain or .gz)");
  a.add("output", "o", false, true,
        "output BAM file (with --disable-merge a directory of bucket BAMs; with --sample_sheet the folder of the "
        "samples' outputs)");
  a.add("sample_sheet", "F", false, false, "sample sheet (#sample_id,fastq1,fastq2,rg,platform_id,library_id) or "
        "folder of *_1.fastq.gz / *_2.fastq.gz");
  a.add("rg", "R", false, false, "read group id ('ID' in BAM header)");
  a.add("sp", "S", false, false, "sample id ('SM' in BAM header)");
  a.add("pl", "P", false, false, "platform id ('PL' in BAM header)");
  a.add("lb", "L", false, false, "library id ('LB' in BAM header)");
  a.add("align-only", "l", true, false, "skip mark duplicates (they are marked only with markdup.in_align=true)");
  a.add("disable-merge", "", true, false, "give bucket bams instead of the whole bam");
  a.add("chains-out", "", false, false, "debug (bwa.seeder=minimizer): write every read's chaining scores, predecessors and kept chains");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome align' options:\n" << a.help();
    throw;
  }
  const std::string ref = a.get("ref"), sheet = a.get("sample_sheet"), fq1 = a.get("fastq1"), fq2 = a.get("fastq2");
  const std::string output = a.get("output");
  const bool force = a.has("force"), disable_merge = a.has("disable-merge"), align_only = a.has("align-only");
  const std::vector<std::string> extra = a.all("extra-options");
  SampleSheetMap samples;
  if (sheet.empty()) {
    if (fq1.empty()) throw invalidParam("Either --sample_sheet or --fastq1,fastq2 needs to be specified");
    SampleDetails d;
    d.fastqR1 = fq1;
    d.fastqR2 = fq2;
    d.ReadGroup = a.get("rg", "sample");
    d.Platform = a.get("pl", "illumina");
    d.LibraryID = a.get("lb", "sample");
    samples[a.get("sp", "sample")].push_back(d);
  } else {
    if (!fq1.empty() || !fq2.empty())
      throw invalidParam("--sample_sheet and --fastq1,fastq2 cannot be specified at the same time");
    samples = read_sample_sheet(sheet);
  }
  if (!is_regular_file(ref)) throw fileNotFound(ref);
  if (sheet.empty() && !disable_merge) {
    if (!force && path_exists(output)) throw invalidParam("output " + output + " exists (use -f)");
  } else {
    if (path_exists(output) && !is_directory(output))
      throw fileNotFound("Output path " + output + " is not a directory");
    create_dir(output);
  }
  AlignRun r;
  r.ref = ref, r.extra = extra, r.force = force, r.disable_merge = disable_merge, r.align_only = align_only;
  r.chains_out = a.get("chains-out");
  const std::vector<int> gpus = slots();
  for (const auto& [sample_id, list] : samples)
    align_sample(r, sample_id, list, sheet.empty() ? output : output + "/" + sample_id + ".bam", !sheet.empty(), gpus);
  return 0;
}

// `fcs-genome germline` (reference src/worker-germline.cpp): FASTQ to GVCF in
// one run.  Per sample: every read group aligned with the minimizer seeder
// (germline.seeder; the reference's minimap-flow), several merged; then the
// stages of `htc` over that BAM.  The BAM stays (<output>.bam) with
// --produce-bam, otherwise it lives under the temp dir.  With -F the outputs
// are <output>/<sample>.{vcf,bam}.  The reference's bucket-BAM hand-off between
// the halves is not restated: htc reads the one sorted BAM.
int germline_main(int argc, char** argv) {
  Args a;
  common_opts(a);
  a.add("ref", "r", false, true, "reference genome path");
  a.add("fastq1", "1", false, false, "input pair-end fastq file (plain or .gz)");
  a.add("fastq2", "2", false, false, "input pair-end fastq file (plain or .gz)");
  a.add("sample_sheet", "F", false, false, "sample sheet or folder");
  a.add("read-group", "R", false, false, "read group id ('ID' in BAM header)");
  a.add("sample-id", "S", false, false, "sample id ('SM' in BAM header)");
  a.add("platform", "P", false, false, "platform id ('PL' in BAM header)");
  a.add("library", "l", false, false, "library id ('LB' in BAM header)");
  a.add("produce-bam", "b", true, false, "keep the sorted BAM (the output with extension .bam)");
  a.add("output", "o", false, true, "output GVCF/VCF file (<output>.gz + .tbi are written too; with --sample_sheet a folder)");
  a.add("produce-vcf", "v", true, false, "produce VCF instead of GVCF");
  a.add("intervalList", "L", false, false, "interval list file");
  a.add("gatk4", "", true, false, "accepted for compatibility");
  a.add("htc-extra-options", "", false, false, "extra options for HaplotypeCaller");
  a.add("chains-out", "", false, false, "debug: write every read's chaining scores, predecessors and kept chains");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome germline' options:\n" << a.help();
    throw;
  }
  const std::string ref = a.get("ref"), sheet = a.get("sample_sheet"), fq1 = a.get("fastq1"), fq2 = a.get("fastq2");
  const std::string output = a.get("output");
  const bool force = a.has("force"), keep_bam = a.has("produce-bam");
  SampleSheetMap samples;
  if (sheet.empty()) {
    if (fq1.empty() || fq2.empty()) throw invalidParam("Either --sample_sheet or --fastq1,fastq2 needs to be specified");
    SampleDetails d;
    d.fastqR1 = fq1, d.fastqR2 = fq2;
    d.ReadGroup = a.get("read-group", "sample"), d.Platform = a.get("platform", "illumina"), d.LibraryID = a.get("library", "sample");
    samples[a.get("sample-id", "sample")].push_back(d);
  } else {
    if (!fq1.empty() || !fq2.empty())
      throw invalidParam("--sample_sheet and --fastq1,fastq2 cannot be specified at the same time");
    samples = read_sample_sheet(sheet);
  }
  if (!is_regular_file(ref)) throw fileNotFound(ref);
  if (!sheet.empty()) {
    if (path_exists(output) && !is_directory(output)) throw fileNotFound("Output path " + output + " is not a directory");
    create_dir(output);
  }
  // <stem>.<ext> of one sample's output
  auto with_ext = [](const std::string& path, const std::string& ext) {
    const size_t dot = path.find_last_of('.'), slash = path.find_last_of('/');
    const bool has = dot != std::string::npos && (slash == std::string::npos || dot > slash + 1);
    return (has ? path.substr(0, dot) : path) + "." + ext;
  };
  const bool flag_vcf = a.has("produce-vcf");
  struct Out {
    std::string vcf, bam;
  };
  std::map<std::string, Out> outs;
  const std::string bam_dir = conf().temp_dir() + "/germline";
  for (const auto& kv : samples) {
    Out o;
    o.vcf = sheet.empty() ? output : output + "/" + kv.first + (flag_vcf ? ".vcf" : ".g.vcf");
    o.bam = keep_bam ? with_ext(o.vcf, "bam") : bam_dir + "/" + kv.first + ".bam";
    if (!force)
      for (const std::string& f : {o.vcf, o.vcf + ".gz", keep_bam ? o.bam : std::string()})
        if (!f.empty() && path_exists(f)) throw invalidParam("output " + f + " exists (use -f)");
    outs[kv.first] = o;
  }
  if (!keep_bam) create_dir(bam_dir);
  AlignRun r;
  r.ref = ref, r.extra = a.all("extra-options"), r.force = force || !keep_bam;
  r.seeder = conf().get_string("germline.seeder"), r.chains_out = a.get("chains-out");
  seeder_from_name(r.seeder);
  const std::vector<int> gpus = slots();
  for (const auto& [sample_id, list] : samples) {
    const Out& o = outs[sample_id];
    align_sample(r, sample_id, list, o.bam, !sheet.empty(), gpus);
    HtcRun h;
    h.ref = ref, h.input = o.bam, h.output = o.vcf, h.intervals = a.get("intervalList"), h.sample_id = sample_id;
    h.extra = a.all("htc-extra-options");
    h.force = force, h.produce_vcf = flag_vcf;
    run_htc(h, gpus);
    if (!keep_bam) {
      std::remove(o.bam.c_str());
      std::remove((o.bam + ".bai").c_str());
    }
  }
  return 0;
}

// What the handlers of markdup, baserecal / printreads / bqsr, depth and ug share.
// fileNotFound unless the path is a regular file (or, for an input of part BAMs, anything that exists).
void require_path(const std::string& path, bool or_directory = false) {
  if (!(or_directory ? path_exists(path) : is_regular_file(path))) throw fileNotFound(path);
}

// Without -f, the first of the command's output files that exists is refused.
void refuse_existing(const Args& a, const std::vector<std::string>& outputs) {
  if (a.has("force")) return;
  for (const std::string& f : outputs)
    if (path_exists(f)) throw invalidParam("output " + f + " exists (use -f)");
}

// The end of a command's stats line on stderr.
void stats_tail(double seconds, bool on_device) {
  std::cerr << ", " << seconds << " s (" << (on_device ? "GPU" : "host") << ")" << std::endl;
}

// `fcs-genome markdup -i in.bam -o out.bam` (reference src/worker-markdup.cpp,
// which runs sambamba markdup): the whole BAM is read into memory, marked as
// one batch (host/markdup.h) and written in its input order.  With
// markdup.gpu=false the command needs no GPU.
int markdup_main(int argc, char** argv) {
  Args a;
  common_opts(a);
  a.add("input", "i", false, true, "input BAM file");
  a.add("output", "o", false, true, "output BAM file (a .bai is written when the input is coordinate-sorted)");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome markdup' options:\n"
              << a.help()
              << "The input is held in memory as a whole (about 2.5x its uncompressed size); "
                 "there is no spilling, out-of-core mode.\n";
    throw;
  }
  const std::string input = a.get("input"), output = a.get("output");
  require_path(input);
  refuse_existing(a, {output});
  int device = -1;
  if (conf().get_bool("markdup.gpu")) device = slots().front();
  const MarkdupStats st = markdup_bam(input, output, device);
  std::cerr << "[fcs-genome markdup] " << st.examined << " records examined, " << st.pairs << " pairs, " << st.fragments
            << " fragments, " << st.duplicates << " records flagged";
  stats_tail(st.seconds, st.on_device);
  return 0;
}

// `fcs-genome baserecal | printreads | bqsr` (reference src/worker-bqsr.cpp:145-330,
// which runs GATK's BaseRecalibrator and PrintReads / ApplyBQSR per contig
// part): the BAM streams through host/bqsr_run.h in chunks, counted and
// rewritten on the GPU (bqsr.gpu=true, include/fcsbq.h) or on the host.  With
// bqsr.gpu=false the commands need no GPU.
enum class BqsrCommand { kBaserecal, kPrintreads, kBqsr };

int bqsr_main(int argc, char** argv, BqsrCommand cmd) {
  const bool counts = cmd != BqsrCommand::kPrintreads, applies = cmd != BqsrCommand::kBaserecal;
  const char* name = cmd == BqsrCommand::kBaserecal ? "baserecal" : cmd == BqsrCommand::kPrintreads ? "printreads" : "bqsr";
  Args a;
  common_opts(a);
  a.add("ref", "r", false, true, "reference genome path");
  a.add("input", "i", false, true, "input BAM file or dir");
  if (cmd == BqsrCommand::kBaserecal) a.add("output", "o", false, true, "output BQSR file");
  else a.add("output", "o", false, true, "output BAM file (a .bai is written when the input is coordinate-sorted)");
  if (counts) a.add("knownSites", "K", false, false, "known sites for base recalibration (VCF or VCF.gz; may repeat)");
  if (cmd == BqsrCommand::kPrintreads) a.add("bqsr", "b", false, true, "input BQSR file");
  if (cmd == BqsrCommand::kBqsr) a.add("bqsr", "b", false, false, "output BQSR file (default: none is written)");
  if (applies) a.add("merge-bam", "m", true, false, "accepted; the output is always one BAM");
  a.add("gatk4", "g", true, false, "accepted; the rules are GATK 4's");
  a.add("sample-id", cmd == BqsrCommand::kBaserecal ? "" : "t", false, false, "sample tag for log files");
  a.add("intervalList", "L", false, false, "interval list file: only the records overlapping it are read");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome " << name << "' options:\n" << a.help();
    throw;
  }
  BqsrJob job;
  job.ref = a.get("ref"), job.input = a.get("input");
  if (a.has("intervalList")) job.intervals = a.get("intervalList");
  require_path(job.ref), require_path(job.input, true);
  if (!job.intervals.empty()) require_path(job.intervals);
  if (counts) {
    job.known = a.all("knownSites");
    for (const std::string& k : job.known) require_path(k);
  }
  const std::string output = a.get("output");
  if (cmd == BqsrCommand::kBaserecal) job.report = output;
  else job.output = output, job.report = a.get("bqsr");
  if (cmd == BqsrCommand::kPrintreads) require_path(job.report);
  refuse_existing(a, cmd == BqsrCommand::kBqsr && !job.report.empty() ? std::vector<std::string>{output, job.report}
                                                                      : std::vector<std::string>{output});
  if (conf().get_bool("bqsr.gpu")) job.device = slots().front();
  const BqsrStats st = cmd == BqsrCommand::kBaserecal ? baserecal_run(job)
                       : cmd == BqsrCommand::kPrintreads ? printreads_run(job) : bqsr_run(job);
  std::cerr << "[fcs-genome " << name << "] " << st.records << " records";
  if (counts)
    std::cerr << ", " << st.counted << " counted, " << st.observations << " observations, " << st.errors << " errors, "
              << st.known_sites << " known sites (" << st.known_skipped << " on unknown contigs)";
  if (applies) std::cerr << ", " << st.recalibrated << " recalibrated";
  stats_tail(st.seconds, st.on_device);
  return 0;
}

// `fcs-genome depth` (reference src/worker-depth.cpp:14-165, which runs GATK 3's
// DepthOfCoverage per contig part and merges the parts' text files): the BAM
// streams through host/depth_run.h in chunks over windows of the genome,
// counted and summarised on the GPU (depth.gpu=true, include/fcsdp.h) or on
// the host.  With depth.gpu=false the command needs no GPU.
int depth_main(int argc, char** argv) {
  Args a;
  common_opts(a);
  a.add("ref", "r", false, true, "reference genome path");
  a.add("input", "i", false, true, "input BAM file or dir (coordinate-sorted)");
  a.add("output", "o", false, true, "output coverage file (<output>.sample_* are written beside it)");
  a.add("intervalList", "L", false, false, "Interval List BED File");
  a.add("geneList", "g", false, false, "list of genes over which the coverage is calculated (refused: gene summaries are not built)");
  a.add("sample-id", "", false, false, "sample tag for log files");
  a.add("omitBaseOutput", "b", true, false, "omit output coverage depth at each base (default: false)");
  a.add("omitIntervals", "v", true, false, "omit output coverage per-interval statistics (default false)");
  a.add("omitSampleSummary", "s", true, false, "omit output summary files for each sample (default false)");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome depth' options:\n" << a.help();
    throw;
  }
  DepthJob job;
  job.ref = a.get("ref"), job.input = a.get("input"), job.output = a.get("output");
  if (a.has("intervalList")) job.intervals = a.get("intervalList");
  if (a.has("sample-id")) (void)a.get("sample-id");
  if (a.has("geneList")) {
    (void)a.get("geneList");
    throw invalidParam("--geneList: gene summaries are not built");
  }
  job.omit_base = a.has("omitBaseOutput"), job.omit_intervals = a.has("omitIntervals");
  job.omit_summary = a.has("omitSampleSummary");
  require_path(job.ref), require_path(job.input, true);
  if (!job.intervals.empty()) require_path(job.intervals);
  refuse_existing(a, depth_output_files(job));
  if (conf().get_bool("depth.gpu")) job.device = slots().front();
  const DepthRunStats st = depth_run(job);
  std::cerr << "[fcs-genome depth] sample " << st.sample << ": " << st.records << " records, " << st.intervals << " intervals, "
            << st.windows << " windows, " << st.loci << " loci, total depth " << st.total;
  stats_tail(st.seconds, st.on_device);
  return 0;
}

// `fcs-genome ug` (reference src/worker-ug.cpp, src/workers/UGWorker.cpp, which
// run GATK 3's UnifiedGenotyper per shard and concatenate the shards' VCFs): the
// BAM streams through host/ug_run.h in chunks gathered per window of the
// genome, piled up on the GPU (ug.gpu=true, include/fcsug.h) or on the host and
// genotyped by the SNP model.  With ug.gpu=false the command needs no GPU.
int ug_main(int argc, char** argv) {
  Args a;
  common_opts(a);
  a.add("ref", "r", false, true, "reference genome path");
  a.add("input", "i", false, true, "input BAM file or dir (coordinate-sorted)");
  a.add("output", "o", false, true, "output VCF file (<output>.gz and <output>.gz.tbi are written beside it)");
  a.add("intervalList", "L", false, false, "Interval List BED File");
  a.add("sample-id", "", false, false, "sample tag for log files");
  a.add("skip-concat", "s", true, false, "produce a set of VCF files instead of one (refused: one run is one stream)");
  a.add("extra-options", "O", false, false, "extra options for GATK (accepted and ignored)");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome ug' options:\n" << a.help();
    throw;
  }
  UgJob job;
  job.ref = a.get("ref"), job.input = a.get("input"), job.output = a.get("output");
  if (a.has("intervalList")) job.intervals = a.get("intervalList");
  if (a.has("sample-id")) (void)a.get("sample-id");
  if (a.has("skip-concat")) throw invalidParam("--skip-concat: one run is one stream and writes one VCF, there are no parts to keep");
  if (a.has("extra-options"))
    std::cerr << "[fcs-genome ug] --extra-options " << a.get("extra-options") << ": ignored (no GATK is run)" << std::endl;
  require_path(job.ref), require_path(job.input, true);
  if (!job.intervals.empty()) require_path(job.intervals);
  refuse_existing(a, ug_output_files(job));
  if (conf().get_bool("ug.gpu")) job.device = slots().front();
  const UgRunStats st = ug_run(job);
  std::cerr << "[fcs-genome ug] sample " << st.sample << ": " << st.records << " records, " << st.intervals << " intervals, "
            << st.windows << " windows, " << st.sites << " sites, " << st.calls << " calls";
  stats_tail(st.seconds, st.on_device);
  return 0;
}

// `fcs-genome joint` (reference src/worker-joint.cpp, which runs GATK's
// CombineGVCFs and GenotypeGVCFs per shard and concatenates the shards' VCFs):
// the directory's one-sample GVCFs stream through host/joint_run.h a contig at
// a time, combined into a site table and genotyped on the GPU (joint.gpu=true,
// include/fcsjg.h) or on the host.  With joint.gpu=false the command needs no GPU.
int joint_main(int argc, char** argv) {
  Args a;
  common_opts(a);
  a.add("ref", "r", false, true, "reference genome path");
  a.add("input-dir", "i", false, true, "directory of one-sample GVCFs (*.gvcf.gz, *.g.vcf.gz, *.gvcf, *.g.vcf), taken in name order");
  a.add("output", "o", false, true, "output VCF file (<output>.gz and <output>.gz.tbi are written beside it)");
  a.add("sample-id", "", false, false, "sample tag for log files");
  a.add("database_name", "", false, false, "database name (accepted and ignored: no GenomicsDB is written)");
  a.add("combine-only", "c", true, false, "stop after the combine step (refused: no combined GVCF is written)");
  a.add("skip-combine", "g", true, false, "start from a combined GVCF (refused: none is read)");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome joint' options:\n" << a.help();
    throw;
  }
  JointJob job;
  job.ref = a.get("ref"), job.input = a.get("input-dir"), job.output = a.get("output");
  if (a.has("sample-id")) (void)a.get("sample-id");
  if (a.has("combine-only")) throw invalidParam("--combine-only: the combine step keeps its table in memory, no combined GVCF is written");
  if (a.has("skip-combine")) throw invalidParam("--skip-combine: the input is a directory of one-sample GVCFs, no combined GVCF is read");
  if (a.has("database_name"))
    std::cerr << "[fcs-genome joint] --database_name " << a.get("database_name") << ": ignored (no GenomicsDB is written)" << std::endl;
  require_path(job.ref);
  if (!is_directory(job.input)) throw fileNotFound(job.input + " (a directory of GVCFs)");
  refuse_existing(a, joint_output_files(job));
  if (conf().get_bool("joint.gpu")) job.device = slots().front();
  const JointRunStats st = joint_run(job);
  std::cerr << "[fcs-genome joint] " << st.samples << " samples, " << st.records << " records, " << st.sites << " sites, "
            << st.written << " written, " << st.clamped << " PLs clamped, " << st.ignored << " calls ignored, " << st.cut
            << " ALTs cut";
  stats_tail(st.seconds, st.on_device);
  return 0;
}

// `fcs-genome indel | ir` (reference src/worker-indel.cpp, src/workers/IndelWorker.cpp
// and RTCWorker.cpp, which run GATK 3's RealignerTargetCreator and IndelRealigner
// per contig part): the sorted BAM streams three times through host/indel_run.h;
// every (consensus, alt read) pair of every target is scored on the GPU
// (indel.gpu=true, include/fcsir.h) or on the host.  With indel.gpu=false the
// command needs no GPU.
int indel_main(int argc, char** argv) {
  Args a;
  common_opts(a);
  a.add("ref", "r", false, true, "reference genome path");
  a.add("input", "i", false, true, "input BAM file or dir (coordinate-sorted)");
  a.add("output", "o", false, true, "output BAM file (a .bai is written beside it)");
  a.add("intervalList", "L", false, false, "interval list file: only the targets overlapping it are realigned");
  a.add("known", "K", false, false, "known indels for realignment (VCF or VCF.gz; may repeat)");
  a.add("merge-bam", "m", true, false, "accepted; the output is always one BAM");
  a.add("sample-id", "", false, false, "sample tag for log files");
  a.add("targets-out", "", false, false, "also write the realignment targets, in GATK's interval format");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome indel' options:\n" << a.help();
    throw;
  }
  IndelJob job;
  job.ref = a.get("ref"), job.input = a.get("input"), job.output = a.get("output");
  if (a.has("intervalList")) job.intervals = a.get("intervalList");
  if (a.has("sample-id")) (void)a.get("sample-id");
  if (a.has("targets-out")) job.targets_out = a.get("targets-out");
  job.known = a.all("known");
  require_path(job.ref), require_path(job.input, true);
  if (!job.intervals.empty()) require_path(job.intervals);
  for (const std::string& k : job.known) require_path(k);
  refuse_existing(a, job.targets_out.empty() ? std::vector<std::string>{job.output} : std::vector<std::string>{job.output, job.targets_out});
  if (conf().get_bool("indel.gpu")) job.device = slots().front();
  const IndelRunStats st = indel_run(job);
  std::cerr << "[fcs-genome indel] " << st.records << " records, " << st.known << " known indels, " << st.targets << " targets, "
            << st.bins << " bins (" << st.untouched << " left untouched), " << st.alt_reads << " alt reads, " << st.pairs
            << " pairs, " << st.cleaned << " bins cleaned, " << st.realigned << " records realigned, " << st.mates << " mates fixed";
  stats_tail(st.seconds, st.on_device);
  return 0;
}

// `fcs-genome index -r ref.fasta`: the aligner's FMD-index, saved next to the
// FASTA (<ref>.fcsidx) so that align maps it instead of building one per run
// (bwa-flow reads the prebuilt bwa index; the reference expects it beside the
// FASTA, src/workers/BWAWorker.cpp:134-147).
int index_main(int argc, char** argv) {
  Args a;
  a.add("ref", "r", false, true, "reference genome path");
  a.add("sa-intv", "", false, false, "suffix-array sampling interval (default: automatic, <= 8 GiB of samples)");
  try {
    a.parse(argc, argv);
  } catch (helpRequest&) {
    std::cerr << "'fcs-genome index' options:\n" << a.help();
    throw;
  }
  const std::string ref = a.get("ref");
  if (!is_regular_file(ref)) throw fileNotFound(ref);
  const uint64_t t0 = now_us();
  build_fmd_index(ref, a.has("sa-intv") ? std::stoi(a.get("sa-intv")) : 0);
  std::cerr << "[fcs-genome index] " << fmd_index_path(ref) << " written in " << (now_us() - t0) / 1e6 << " s"
            << std::endl;
  return 0;
}

int synth_main(int argc, char** argv) {
  Args a;
  a.add("output", "o", false, true, "output directory");
  a.add("contigs", "c", false, false, "name:length[,name:length...] (default chr20:1000000)");
  a.add("coverage", "x", false, false, "sample coverage (default 30)");
  a.add("seed", "s", false, false, "seed (default 20261015)");
  a.add("max-reads", "n", false, false, "keep only the first N reads by position (C1: 1000)");
  a.add("tumor", "T", true, false, "also write tumor.bam with somatic variants (C5)");
  a.add("tumor-coverage", "", false, false, "tumor coverage (default 40)");
  a.add("somatic-af", "", false, false, "somatic allele fraction (default 0.3)");
  a.add("noisy-frac", "", false, false, "fraction of reads drawn with 20% high-quality mismatches (mis-mapped-like)");
  a.add("spike", "", false, false, "chr:pos[,chr:pos...] plant three het SNVs at pos-30, pos, pos+30 (1-based)");
  a.add("parts", "", false, false, "also split the sample into parts/part-XXXXXX.bam + .bed (N buckets)");
  a.add("paired", "", false, false, "also write sample_1/2.fastq: FR pairs with fragment length ~ N(ARG, 50)");
  a.add("no-fastq", "", true, false, "do not write sample.fastq (the single-end FASTQ of the sample's reads)");
  a.parse(argc, argv);
  SynthSpec sp;
  if (a.has("contigs")) {
    sp.contigs.clear();
    std::string s = a.get("contigs");
    size_t p = 0;
    while (p < s.size()) {
      const size_t e = std::min(s.find(',', p), s.size());
      const std::string tok = s.substr(p, e - p);
      const size_t c = tok.find(':');
      if (c == std::string::npos) throw invalidParam("--contigs " + s);
      sp.contigs.emplace_back(tok.substr(0, c), std::stoll(tok.substr(c + 1)));
      p = e + 1;
    }
  }
  if (a.has("spike")) {
    std::string s = a.get("spike");
    for (size_t p = 0; p < s.size();) {
      const size_t e = std::min(s.find(',', p), s.size());
      const std::string tok = s.substr(p, e - p);
      const size_t c = tok.rfind(':');
      if (c == std::string::npos) throw invalidParam("--spike " + s);
      sp.spikes.emplace_back(tok.substr(0, c), std::stoll(tok.substr(c + 1)) - 1);
      p = e + 1;
    }
  }
  if (a.has("no-fastq")) sp.single_fastq = false;
  if (a.has("noisy-frac")) sp.noisy_frac = std::stod(a.get("noisy-frac"));
  if (a.has("parts")) sp.parts = std::stoi(a.get("parts"));
  if (a.has("paired")) sp.paired_insert = std::stoi(a.get("paired"));
  if (a.has("coverage")) sp.coverage = std::stod(a.get("coverage"));
  if (a.has("seed")) sp.seed = std::stoull(a.get("seed"));
  if (a.has("max-reads")) sp.max_reads = std::stoll(a.get("max-reads"));
  if (a.has("tumor")) sp.somatic_rate = 1e-4;
  if (a.has("tumor-coverage")) sp.tumor_coverage = std::stod(a.get("tumor-coverage"));
  if (a.has("somatic-af")) sp.somatic_af = std::stod(a.get("somatic-af"));
  const SynthOutputs o = synth_dataset(sp, a.get("output"));
  std::cout << "{\"ref\": \"" << o.ref_fasta << "\", \"bam\": \"" << o.bam << "\", \"fastq\": \"" << o.fastq
            << "\", \"truth\": \"" << o.truth_vcf << "\", \"tumor_bam\": \"" << o.tumor_bam
            << "\", \"parts\": \"" << o.parts_dir << "\", \"fastq1\": \"" << o.fastq1 << "\", \"fastq2\": \""
            << o.fastq2 << "\", \"pairs_truth\": \"" << o.pairs_truth
            << "\", \"reads\": " << o.n_reads << ", \"tumor_reads\": " << o.n_tumor_reads
            << ", \"variants\": " << o.variants.size() << "}" << std::endl;
  return 0;
}

// SIGINT / SIGTERM / SIGHUP (the reference's sigint_handler, src/main.cpp:43-54):
// an async-signal-safe handler writes the signal number to a pipe, and a
// watcher thread announces the interrupt and sets the flag the Executor and
// the workers poll; the run then unwinds, removes its temp dir and exits
// 128 + signal.  A second signal exits at once.  No signal is blocked, so the
// threads of the HIP runtime and of a profiler (rocprofv3) see the process's
// signals as they would without fcs-genome's handling (round 2 blocked the
// three signals in every thread, and a profiled run hung at exit).
int g_sig_pipe[2] = {-1, -1};
volatile sig_atomic_t g_sig_seen = 0;

extern "C" void on_signal(int sig) {
  if (g_sig_seen) _exit(128 + sig);
  g_sig_seen = sig;
  const unsigned char b = (unsigned char)sig;
  if (write(g_sig_pipe[1], &b, 1) < 0) _exit(128 + sig);
}

void start_signal_thread() {
  if (pipe(g_sig_pipe) != 0) return;
  std::thread([] {
    unsigned char b = 0;
    for (;;) {
      const ssize_t n = read(g_sig_pipe[0], &b, 1);
      if (n == 1) break;
      if (n < 0 && errno == EINTR) continue;
      return;
    }
    std::cerr << "[fcs-genome] Caught interrupt, cleaning up..." << std::endl;
    set_interrupted((int)b);
  }).detach();
  struct sigaction sa;
  std::memset(&sa, 0, sizeof sa);
  sa.sa_handler = on_signal;
  sigemptyset(&sa.sa_mask);
  sa.sa_flags = SA_RESTART;
  for (int sig : {SIGINT, SIGTERM, SIGHUP}) sigaction(sig, &sa, nullptr);
}

int print_help() {
  std::cout << "Falcon Genome Analysis Toolkit (MI355X / gfx950 build)\n"
               "Usage: fcs-genome [command] <options>\n\nCommands:\n"
               "  align           align FASTQ reads into a sorted BAM (GPU banded SW)\n"
               "  germline        FASTQ to GVCF in one run: minimizer-seeded align, then htc\n"
               "  markdup         mark duplicate reads of a BAM (GPU sort + segmented arg-max)\n"
               "  indel           indel realignment of a BAM, IndelRealigner-style (GPU consensus scoring)\n"
               "  baserecal       base recalibration table of a BAM against known sites (GPU covariate counting)\n"
               "  printreads      apply a base recalibration table to a BAM (GPU table lookup)\n"
               "  bqsr            baserecal and printreads in one run\n"
               "  depth           depth of coverage of a BAM per locus, interval and sample (GPU difference array + scan)\n"
               "  ug              SNP calling from the pileup, UnifiedGenotyper-style (GPU pileup in LDS tiles)\n"
               "  htc             variant calling, HaplotypeCaller-style (GPU PairHMM)\n"
               "  joint           joint genotyping of htc's GVCFs (GPU exact allele-frequency model)\n"
               "  mutect2         somatic variant calling, tumor/normal (GPU PairHMM)\n"
               "  conf            print configuration keys\n"
               "  index           build the aligner's FMD-index of a reference (<ref>.fcsidx)\n"
               "  synth           write synthetic reference/BAM/FASTQ/truth inputs\n";
  return 0;
}

}  // namespace
}  // namespace fcsg

int main(int argc, char** argv) {
  using namespace fcsg;
  if (argc < 2) {
    print_help();
    return 1;
  }
  std::string cmd = argv[1];
  for (char& c : cmd) c = (char)std::tolower((unsigned char)c);
  int ret = 0;
  std::string root;
  {
    std::string self = argv[0];
    const size_t k = self.find_last_of('/');
    root = k == std::string::npos ? "." : self.substr(0, k) + "/..";
  }
  timeline("main");
  // Shard threads allocate and free large blocks in batches (PairHMM region
  // batches, per-window vectors): keep freed memory in the allocator instead
  // of returning it (munmap / heap trim) only to fault it back in — with 32
  // threads in one process those faults serialize on the memory-map lock.
  mallopt(M_MMAP_THRESHOLD, 256 << 20);
  mallopt(M_TRIM_THRESHOLD, 1 << 30);
  start_signal_thread();
  try {
    conf().init(root);
    if (cmd == "htc") ret = htc_main(argc - 1, argv + 1);
    else if (cmd == "mutect2") ret = mutect2_main(argc - 1, argv + 1);
    else if (cmd == "align" || cmd == "al") ret = align_main(argc - 1, argv + 1);
    else if (cmd == "germline" || cmd == "gm") ret = germline_main(argc - 1, argv + 1);
    else if (cmd == "markdup" || cmd == "md") ret = markdup_main(argc - 1, argv + 1);
    else if (cmd == "baserecal") ret = bqsr_main(argc - 1, argv + 1, BqsrCommand::kBaserecal);
    else if (cmd == "printreads" || cmd == "pr") ret = bqsr_main(argc - 1, argv + 1, BqsrCommand::kPrintreads);
    else if (cmd == "bqsr") ret = bqsr_main(argc - 1, argv + 1, BqsrCommand::kBqsr);
    else if (cmd == "depth") ret = depth_main(argc - 1, argv + 1);
    else if (cmd == "ug" || cmd == "unifiedgeno") ret = ug_main(argc - 1, argv + 1);
    else if (cmd == "joint") ret = joint_main(argc - 1, argv + 1);
    else if (cmd == "indel" || cmd == "ir") ret = indel_main(argc - 1, argv + 1);
    else if (cmd == "synth") ret = synth_main(argc - 1, argv + 1);
    else if (cmd == "index") ret = index_main(argc - 1, argv + 1);
    else if (cmd == "conf") {
      std::cerr << "fcs-genome configuration options:\n" << conf().dump();
      ret = 1;  // the reference exits through silentExit here
    } else if (cmd == "--version") {
      std::cout << "fcs-genome (gfx950) / " << fcs_version() << std::endl;
    } else {
      print_help();
      ret = 1;
    }
    remove_path(conf().temp_dir());
    timeline("temp removed");
  } catch (helpRequest&) {
    ret = 0;
  } catch (invalidParam& e) {
    std::cerr << "[fcs-genome] ERROR: Failed to parse arguments: invalid option " << e.what() << std::endl;
    ret = 1;
  } catch (pathEmpty& e) {
    std::cerr << "[fcs-genome] ERROR: Failed to parse arguments: option " << e.what() << " cannot be empty" << std::endl;
    ret = 1;
  } catch (fileNotFound& e) {
    std::cerr << "[fcs-genome] ERROR: " << e.what() << std::endl;
    ret = 3;
  } catch (silentExit&) {
    ret = 1;
  } catch (interruptedError&) {
    remove_path(conf().temp_dir());
    ret = 128 + interrupt_signal();
  } catch (failedCommand& e) {
    if (*e.what()) std::cerr << e.what() << std::endl;
    ret = 4;
  } catch (std::runtime_error& e) {
    std::cerr << "[fcs-genome] ERROR: Encountered an error: " << e.what() << std::endl;
    ret = -1;
  }
  timeline("exit");
  // Every output is closed; flush the streams and leave without running static
  // destructors or the GPU runtime's teardown (≈ 0.3 s of unloading and
  // freeing after the last output on the bench box); the kernel reclaims the
  // process's memory and devices as it does for any exit.
  std::cout.flush();
  std::cerr.flush();
  std::fflush(nullptr);
#if defined(__SANITIZE_ADDRESS__) || defined(__SANITIZE_THREAD__)
  return ret;  // sanitizer builds keep the normal exit (leak and race reports run at exit)
#else
  if (std::getenv("FCS_NORMAL_EXIT")) return ret;  // profilers that report from atexit handlers
  std::_Exit(ret);
#endif
}
