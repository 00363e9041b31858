#include "config.h"

#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <thread>

#include "common.h"
#include "fcship.h"

namespace fcsg {

Config& Config::global() {
  static Config c;
  return c;
}

void Config::declare(const std::string& key, const std::string& def, const std::string& help) {
  kv_[key] = Entry{def, help, false};
}

void Config::init(const std::string& root_dir) {
  kv_.clear();
  const unsigned ncpu = host_cpus();
  // common (config.cpp:274-296)
  declare("temp_dir", "/tmp", "temp dir for fast access");
  declare("log_dir", "./log", "log dir");
  declare("hosts", "", "host list for scale-out mode");
  declare("latency_mode", "false", "enable latency mode");
  // tools (config.cpp:298-353), the GATK/BWA knobs that still mean something here
  declare("bwa.verbose", "0", "verbose level of the aligner");
  declare("bwa.nt", "-1", "host threads of the aligner (-1: all)");
  declare("bwa.num_buckets", "1024", "number of BAM buckets");
  declare("bwa.chunk_size", "100000", "reads per SW batch handed to the GPU");
  declare("bwa.seeder", "smem", "the aligner's seeder: smem (FMD-index SMEMs) | minimizer (minimizer anchors, chained)");
  declare("bwa.gpu_seed", "false",
          "collect SMEMs and locate their occurrences on the GPU (one call each per chunk) instead of on the host threads");
  declare("bwa.gpu_seed_fused", "true",
          "with bwa.gpu_seed: one fused call per chunk (order, expand and locate on the GPU, compacted copy back) instead of two");
  declare("bwa.gpu_slots", "0", "aligner host threads (chunks in flight) per GPU; 0: host threads / GPUs, at least 4");
  declare("gatk.intv.path", "", "default path to existing contig intervals");
  declare("gatk.ncontigs", "32", "contig partition num in htc/mutect2");
  declare("gatk.nprocs", std::to_string(std::min(32u, ncpu)), "default concurrent shard tasks");
  declare("gatk.htc.nprocs", "", "concurrent shard tasks in htc (default gatk.nprocs)");
  declare("gatk.mutect2.nprocs", "", "concurrent shard tasks in mutect2 (default gatk.nprocs)");
  declare("gatk.skip_pseudo_chr", "true", "skip pseudo chromosome intervals (contigs after the 25th)");
  // accelerator (replaces bwa.use_fpga / bwa.fpga.bit_path / blaze.nam_path)
  declare("gpu.devices", "all", "GPU ordinals for shard tasks: all | comma list");
  declare("gpu.phmm.batch_regions", "4096", "active regions per PairHMM device pass");
  declare("gpu.phmm.combine_ms", "0", "ms a shard's PairHMM pass waits to merge with other shards' (0: no merging)");
  declare("gpu.phmm.rescue", "true", "fp64 rescue of pairs whose fp32 likelihood underflows (GKL)");
  declare("gpu.release_early", "true",
          "release the GPUs beside the VCF tail once the callers are done (their teardown off the critical path)");
  declare("gpu.warmup_help", "false",
          "a shard whose PairHMM pass finds the GPU runtime still coming up runs a queued shard meanwhile");
  declare("gpu.bam_inflate", "false",
          "inflate a calling window's BAM blocks on the GPU (fcs_bgzf_inflate) instead of host libdeflate");
  declare("gpu.bgzf_deflate", "false",
          "compress the final VCF.gz's and align's BAM blocks on the GPU (fcs_bgzf_deflate) instead of host libdeflate");
  declare("markdup.in_align", "false",
          "align marks duplicates in each read group before the coordinate sort (unless --align-only)");
  declare("markdup.gpu", "false",
          "mark duplicates on the GPU (fcsdup_mark) instead of on the host (markdup, and align with markdup.in_align)");
  declare("bqsr.gpu", "false",
          "count covariates and rewrite qualities on the GPU (fcsbq_count / fcsbq_apply) instead of on the host (baserecal, printreads, bqsr)");
  declare("bqsr.chunk_records", "1000000", "BAM records per chunk of baserecal / printreads / bqsr (one device call each)");
  declare("depth.gpu", "false",
          "count depths and summarise windows on the GPU (fcsdp_count / fcsdp_stats) instead of on the host (depth)");
  declare("depth.chunk_records", "1000000", "BAM records per chunk of depth (one device call per chunk and window)");
  declare("depth.window_bp", "67108864", "loci per window of depth at most (one depth array each; DESIGN 4.11)");
  declare("depth.min_mapq", "-1", "depth: records with a lower MAPQ are not counted");
  declare("depth.max_mapq", "2147483647", "depth: records with a higher MAPQ are not counted");
  declare("depth.min_baseq", "-1", "depth: bases with a lower quality are not counted");
  declare("depth.max_baseq", "127", "depth: bases with a higher quality are not counted");
  declare("depth.include_deletions", "false", "depth: every deleted position adds 1");
  declare("depth.include_ref_n", "false", "depth: loci whose reference base is N take part");
  declare("ug.gpu", "false", "pile sites up on the GPU (fcsug_sites) instead of on the host (ug)");
  declare("ug.chunk_records", "1000000", "BAM records read at a time by ug");
  declare("ug.window_bp", "1048576", "loci per window of ug at most (one device call each; DESIGN 4.12)");
  declare("ug.min_baseq", "17", "ug: bases whose min(quality, MAPQ, 93) is lower are not counted");
  declare("ug.stand_call_conf", "10", "ug: calls with a lower QUAL are not written");
  declare("ug.heterozygosity", "0.001", "ug: the genotype prior's heterozygosity");
  declare("ug.pcr_error", "0.0001", "ug: the PCR error rate folded into every base's error");
  declare("ug.max_deletion_fraction", "0.05", "ug: sites where more than this fraction of the reads has a deletion are not called");
  declare("joint.gpu", "false", "genotype sites on the GPU (fcsjg_genotype) instead of on the host (joint)");
  declare("joint.stand_call_conf", "10", "joint: sites with a lower QUAL are not written");
  declare("joint.heterozygosity", "0.001", "joint: the allele-count prior's heterozygosity");
  declare("joint.max_alt", "6", "joint: ALTs kept per site, the most named first (at most 6)");
  declare("joint.chunk_sites", "0", "joint: sites per genotyping call (0: as many as return 2^24 PLs at most)");
  declare("germline.seeder", "minimizer", "germline: the aligner's seeder (minimizer | smem)");
  declare("minimap.k", "21", "minimizer seeding: k-mer length (4 to 31)");
  declare("minimap.w", "11", "minimizer seeding: k-mers per window");
  declare("minimap.max_occ", "500", "minimizer seeding: a minimizer with more occurrences yields no anchors");
  declare("minimap.max_gap", "100", "minimizer chaining: the largest step between chained anchors, on the read and on the reference");
  declare("minimap.bw", "50", "minimizer chaining: the largest diagonal step between chained anchors");
  declare("minimap.min_cnt", "2", "minimizer chaining: anchors of a kept chain, at least");
  declare("minimap.min_score", "20", "minimizer chaining: score of a kept chain, at least");
  declare("minimap.gpu_chain", "false", "run the chaining recurrence of a chunk on the GPU (fcsmm_chain) instead of on the host threads");
  declare("indel.gpu", "false", "score (consensus, read) pairs on the GPU (fcsir_score) instead of on the host (indel)");
  declare("indel.chunk_pairs", "1048576", "indel: (consensus, read) pairs per scoring call (a bin is never split)");
  declare("indel.max_reads", "20000", "indel: a bin with more cleanable records is left untouched");
  declare("indel.max_consensuses", "30", "indel: consensuses kept per bin, the first ones");
  declare("indel.max_isize", "3000", "indel: a paired record with a larger |TLEN| is not realigned");
  declare("indel.lod_tenths", "50", "indel: the least improvement of a bin's mismatch sum, in tenths (LOD 5.0)");
  // caller knobs (GATK HaplotypeCaller / Mutect2 argument defaults)
  declare("htc.min_base_quality", "10", "min base quality counted as evidence of activity");
  declare("htc.base_quality_threshold", "18", "PairHMM: base quals below this become 6");
  declare("htc.pcr_indel_model", "CONSERVATIVE",
          "GATK --pcr-indel-model: NONE, HOSTILE, AGGRESSIVE, CONSERVATIVE (gap-open caps in tandem repeats)");
  declare("htc.min_mapq", "20", "reads below this mapping quality are ignored");
  declare("htc.active_fraction", "0.15", "mismatch/indel fraction that makes a site active");
  declare("mutect2.active_fraction", "0.10", "tumor mismatch/indel fraction that makes a site active (mutect2)");
  declare("htc.gpu_pileup", "false",
          "pile a calling window's aligned bases up on the GPU (fcspu_pile) instead of on the shard's host thread (htc, mutect2)");
  declare("htc.pileup_chunk_bp", "1048576", "loci per fcspu_pile call with htc.gpu_pileup (DESIGN 4.15)");
  declare("htc.padding", "50", "bases added either side of an active site");
  declare("htc.max_region", "300", "max active region length");
  declare("htc.max_reads_per_region", "250", "downsampling cap per region");
  declare("mutect2.tlod", "6.3", "tumor LOD threshold");
  declare("mutect2.nlod", "2.2", "normal LOD threshold");
  declare("root_dir", root_dir, "install root");

  if (!root_dir.empty()) load_file(root_dir + "/fcs-genome.conf", false);  // 3rd priority
  load_file("fcs-genome.conf", true);                                       // 2nd priority
  load_env();                                                               // 1st priority

  const char* user = std::getenv("USER");
  temp_dir_ = get_string("temp_dir") + "/fcs-genome-" + (user ? user : "root") + "-" + std::to_string(getpid());
}

void Config::load_file(const std::string& path, bool override_existing) {
  std::ifstream in(path);
  if (!in) return;
  std::string line, section;
  while (std::getline(in, line)) {
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    auto trim = [](std::string s) {
      s.erase(0, s.find_first_not_of(" \t\r"));
      s.erase(s.find_last_not_of(" \t\r") + 1);
      return s;
    };
    line = trim(line);
    if (line.empty()) continue;
    if (line.front() == '[' && line.back() == ']') {
      section = trim(line.substr(1, line.size() - 2));
      continue;
    }
    const size_t eq = line.find('=');
    if (eq == std::string::npos) throw invalidParam("config line '" + line + "' in " + path);
    std::string key = trim(line.substr(0, eq));
    if (!section.empty()) key = section + "." + key;
    if (!kv_.count(key)) throw invalidParam("unknown config key '" + key + "' in " + path);
    Entry& e = kv_[key];
    if (e.set_explicitly && !override_existing) continue;
    e.value = trim(line.substr(eq + 1));
    e.set_explicitly = true;
  }
}

void Config::load_env() {
  for (auto& kv : kv_) {
    std::string env = "FCS_" + kv.first;
    std::transform(env.begin(), env.end(), env.begin(), [](char c) { return c == '.' ? '_' : (char)std::toupper(c); });
    const char* v = std::getenv(env.c_str());
    if (v) {
      kv.second.value = v;
      kv.second.set_explicitly = true;
    }
  }
}

bool Config::has(const std::string& key) const {
  auto it = kv_.find(key);
  return it != kv_.end() && !it->second.value.empty();
}

std::string Config::get_string(const std::string& key) const {
  auto it = kv_.find(key);
  if (it == kv_.end()) throw invalidParam("unknown config key " + key);
  return it->second.value;
}

int Config::get_int(const std::string& key) const {
  const std::string v = get_string(key);
  try {
    return std::stoi(v);
  } catch (...) {
    throw invalidParam(key + " = '" + v + "' is not an integer");
  }
}

int Config::get_int(const std::string& key, const std::string& fallback) const {
  return has(key) ? get_int(key) : get_int(fallback);
}

bool Config::get_bool(const std::string& key) const {
  std::string v = get_string(key);
  std::transform(v.begin(), v.end(), v.begin(), ::tolower);
  if (v == "true" || v == "1" || v == "yes" || v == "on") return true;
  if (v == "false" || v == "0" || v == "no" || v == "off" || v.empty()) return false;
  throw invalidParam(key + " = '" + v + "' is not a boolean");
}

void Config::set(const std::string& key, const std::string& value) {
  if (!kv_.count(key)) throw invalidParam("unknown config key " + key);
  kv_[key].value = value;
  kv_[key].set_explicitly = true;
}

std::string Config::dump() const {
  std::ostringstream ss;
  for (const auto& kv : kv_)
    ss << "  " << kv.first << " = " << kv.second.value << (kv.second.help.empty() ? "" : "    # " + kv.second.help)
       << '\n';
  return ss.str();
}

std::vector<int> Config::gpu_devices() const {
  const std::string v = get_string("gpu.devices");
  std::vector<int> out;
  if (v.empty() || v == "all") {
    const int n = fcs_device_count();
    for (int i = 0; i < n; ++i) out.push_back(i);
    return out;
  }
  std::stringstream ss(v);
  std::string tok;
  while (std::getline(ss, tok, ',')) {
    if (tok.empty()) continue;
    try {
      out.push_back(std::stoi(tok));
    } catch (...) {
      throw invalidParam("gpu.devices = '" + v + "'");
    }
  }
  return out;
}

}  // namespace fcsg
