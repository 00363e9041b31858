// Duplicate marking (DESIGN §2 [EXT], §4.9): Picard MarkDuplicates' criteria
// as sambamba restates them (the reference's `markdup` command runs sambamba:
// /root/reference/src/worker-markdup.cpp, and its `align` marks inside bwa-flow
// unless --align-only: src/workers/BWAWorker.cpp:154).  [EXT] parity is
// unpinned: neither tool is vendored.
//
// A batch is every record of one read-group job or of one BAM, held in memory.
// mark_duplicates_host is the scalar statement of the rules with std::sort:
// the oracle of the device path (include/fcsdup.h) and the path taken without
// it.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "bam.h"
#include "fcsdup.h"

namespace fcsg {

struct MarkdupStats {
  int64_t examined = 0, pairs = 0, fragments = 0, duplicates = 0;
  double seconds = 0;
  bool on_device = false;
};

// The rules on a flat batch (fcsdup_batch over host arrays); dup[r] = 1 for
// the records to flag.  Throws invalidParam on offsets or mates out of range.
MarkdupStats mark_duplicates_host(const fcsdup_batch& b, uint8_t* dup);
// What the host path computes per record on the way (tools/micro/markdup_test.cpp
// compares csrc/md_keys.h with it): the unclipped 5' position and the score
// of every record, examined or not.
void markdup_host_ends(const fcsdup_batch& b, std::vector<int64_t>& u5, std::vector<uint32_t>& score);

// mate[r]: the primary record of the template's other read (same name, the
// other of read1 / read2), for primary records of paired reads; -1 otherwise.
std::vector<int32_t> match_mates(const std::vector<BamRecord>& recs);

// The loaded libfcship has fcsdup_mark (the tests' CPU mock has not).
bool gpu_markdup_available();

// Marks the batch: matches mates, flattens, runs fcsdup_mark on `device` (or
// the host path when device < 0 or the entry point is missing, with one log
// line in the latter case), then sets 0x400 of every examined record from the
// result (an incoming flag is cleared); other records keep theirs.
// lib[r] in [0, n_lib): the record's library; n_ref: reference sequences.
MarkdupStats mark_duplicates(std::vector<BamRecord>& recs, const std::vector<int32_t>& lib, int32_t n_lib, int32_t n_ref,
                             int device);

// Library index of every record from the header's @RG lines (ID -> LB) and the
// records' RG tags; records without a read group, and read groups without LB,
// share library 0.  Returns the library count.
int32_t libraries_of(const BamHeader& h, const std::vector<BamRecord>& recs, std::vector<int32_t>& lib);

// `fcs-genome markdup`: the whole BAM in memory, marked, written in input
// order (with a .bai when the header says SO:coordinate).
MarkdupStats markdup_bam(const std::string& input, const std::string& output, int device);

}  // namespace fcsg
