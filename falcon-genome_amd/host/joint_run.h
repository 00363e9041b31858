// The joint command around the rules of joint.h: the directory's GVCFs, the
// reference's contigs, one contig of all samples resident at a time, the device
// call (include/fcsjg.h) or the host path per chunk of sites, the shared emit
// step and the VCF with its bgzipped copy and tabix index.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace fcsg {

struct JointJob {
  std::string ref;     // FASTA
  std::string input;   // a directory of one-sample GVCFs
  std::string output;  // <output>, <output>.gz and <output>.gz.tbi
  int device = -1;     // < 0: the host path
};

struct JointRunStats {
  int64_t samples = 0, records = 0, sites = 0, written = 0, clamped = 0, ignored = 0, cut = 0;
  double seconds = 0;
  bool on_device = false;
};

// The loaded libfcship has the fcsjg_* entry points (the tests' CPU mock has not).
bool gpu_joint_available();

// The files the job writes.
std::vector<std::string> joint_output_files(const JointJob& job);

JointRunStats joint_run(const JointJob& job);

}  // namespace fcsg
