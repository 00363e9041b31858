// The joint command (joint_run.h): every GVCF of the directory is opened and
// its header checked; contig by contig, each sample's records are read (on
// threads), combined into the contig's site table, genotyped in chunks of
// sites and written.
#include "joint_run.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <memory>
#include <set>

#include "common.h"
#include "config.h"
#include "fasta.h"
#include "fcship.h"
#include "flat_batch.h"
#include "gvcf.h"
#include "joint.h"
#include "vcf.h"

namespace fcsg {

namespace {

struct JointApi {
  decltype(&fcsjg_genotype) genotype = FCSG_DEVICE_ENTRY(fcsjg_genotype);
};

const JointApi& joint_api() {
  static const JointApi A;
  return A;
}

double conf_number(const std::string& key) {
  const std::string v = conf().get_string(key);
  char* end = nullptr;
  const double d = std::strtod(v.c_str(), &end);
  if (v.empty() || *end) throw invalidParam(key + " = " + v + " is not a number");
  return d;
}

// PLs a call may return: its chunk of sites holds at most this many (sites x samples x genotypes).
constexpr int64_t kChunkPls = (int64_t)1 << 24;

}  // namespace

bool gpu_joint_available() {
  const JointApi& a = joint_api();
  return a.genotype && last_error_entry();
}

std::vector<std::string> joint_output_files(const JointJob& job) {
  return {job.output, job.output + ".gz", job.output + ".gz.tbi"};
}

JointRunStats joint_run(const JointJob& job) {
  const uint64_t t0 = now_us();
  JointRunStats st;
  const int device = device_or_host(job.device, gpu_joint_available(),
                                    "[fcs-genome joint] joint.gpu: the loaded libfcship has no fcsjg_genotype entry point; "
                                    "sites are genotyped on the host\n");
  JointParams prm;
  prm.stand_call_conf = conf_number("joint.stand_call_conf"), prm.heterozygosity = conf_number("joint.heterozygosity");
  prm.max_alt = conf().get_int("joint.max_alt");
  if (prm.max_alt < 1 || prm.max_alt > FCSJG_ALTS_MAX)
    throw invalidParam("joint.max_alt " + std::to_string(prm.max_alt) + " is outside 1 .. " + std::to_string(FCSJG_ALTS_MAX));
  const int chunk_conf = conf().get_int("joint.chunk_sites");
  if (chunk_conf < 0) throw invalidParam("joint.chunk_sites " + std::to_string(chunk_conf));
  const std::vector<std::string> files = gvcf_files(job.input);
  if (files.empty()) throw invalidParam("--input " + job.input + " holds no *.gvcf.gz, *.g.vcf.gz, *.gvcf or *.g.vcf file");
  if (files.size() > FCSJG_SAMPLES_MAX)
    throw invalidParam("--input " + job.input + " holds " + std::to_string(files.size()) + " GVCFs, more than " + std::to_string(FCSJG_SAMPLES_MAX));
  std::vector<std::pair<std::string, int64_t>> contigs;
  {
    const Reference ref = load_fasta(job.ref);
    for (const Contig& c : ref.contigs) {
      if (c.seq.size() > (size_t)INT32_MAX) throw invalidParam("contig " + c.name + " is longer than 2^31 - 1 bases");
      contigs.emplace_back(c.name, (int64_t)c.seq.size());
    }
  }
  std::vector<std::unique_ptr<GvcfReader>> readers;
  for (const std::string& f : files) readers.emplace_back(new GvcfReader(f, contigs));
  std::stable_sort(readers.begin(), readers.end(), [](const auto& a, const auto& b) { return a->sample() < b->sample(); });
  std::vector<std::string> samples;
  for (size_t k = 0; k < readers.size(); ++k) {
    if (k && readers[k]->sample() == readers[k - 1]->sample())
      throw failedCommand("[E::joint] " + readers[k]->path() + " and " + readers[k - 1]->path() + " both hold sample " + readers[k]->sample());
    samples.push_back(readers[k]->sample());
  }
  const int n = (int)readers.size();
  st.samples = n;
  const JointTables tables = joint_tables(prm, n);
  const fcsjg_model model = tables.view();
  const int64_t chunk = chunk_conf > 0 ? chunk_conf : std::max<int64_t>(1, kChunkPls / ((int64_t)n * FCSJG_GENOTYPES_MAX));
  try {
    VcfWriter out(job.output, joint_vcf_header(samples, contigs));
    std::vector<GvcfContig> parts((size_t)n);
    JointContig contig;
    JointSlice slice;
    JointOutputs res;
    std::string text;
    for (size_t ci = 0; ci < contigs.size(); ++ci) {
      std::vector<std::exception_ptr> refused((size_t)n);
      parallel_tasks((size_t)n, host_threads(), [&](size_t s) {
        try {
          readers[s]->read_contig((int)ci, parts[s]);
        } catch (...) {
          refused[s] = std::current_exception();
        }
      });
      for (const std::exception_ptr& e : refused)  // the first in column order
        if (e) std::rethrow_exception(e);
      joint_combine(parts, prm.max_alt, contig);
      st.records += (int64_t)contig.beg.size(), st.sites += (int64_t)contig.n_sites(), st.cut += contig.cut;
      for (size_t lo = 0; lo < contig.n_sites(); lo += (size_t)chunk) {
        const size_t hi = std::min(contig.n_sites(), lo + (size_t)chunk);
        joint_slice(contig, lo, hi, slice);
        const fcsjg_cohort cohort = slice.cohort();
        const fcsjg_sites sites = slice.sites();
        res.resize(sites.n_sites, n, sites.n_sites * n * FCSJG_GENOTYPES_MAX);
        const fcsjg_out o = res.view();
        if (device >= 0) device_check(joint_api().genotype(device, &cohort, &sites, &model, &o), "joint", "fcsjg_genotype");
        else joint_genotype_host(cohort, sites, model, host_threads(), o);
        text.clear();
        st.written += joint_emit(contigs[ci].first, contig, lo, cohort, sites.n_sites, o, text);
        out.write_text(text);
        if (interrupted()) throw interruptedError();
      }
    }
    for (auto& r : readers) r->finish(), st.clamped += r->clamped(), st.ignored += r->ignored();
    out.close();
    bgzip_tabix_file(job.output, job.output + ".gz");
  } catch (...) {  // a refused run leaves no partial file
    for (const std::string& f : joint_output_files(job)) remove_path(f);
    throw;
  }
  st.on_device = device >= 0;
  st.seconds = (now_us() - t0) / 1e6;
  return st;
}

}  // namespace fcsg
