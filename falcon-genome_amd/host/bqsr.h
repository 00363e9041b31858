// Base quality recalibration (DESIGN §2 [EXT], §4.10): GATK 4's
// BaseRecalibrator and ApplyBQSR at their defaults (the reference's baserecal /
// printreads / bqsr commands run GATK: src/worker-bqsr.cpp,
// src/workers/BQSRWorker.cpp).  [EXT] parity is unpinned: GATK is not vendored.
//
// This file states the rules with plain loops over a flat batch
// (include/fcsbq.h): the oracle of the device path and the path taken without
// it.  The commands around it are in bqsr_run.cpp.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "fcsbq.h"

namespace fcsg {

// The reference the rules read: contig bytes one after the other, their starts,
// and the known-sites bitmap (bit g & 63 of word g >> 6).
struct BqRefView {
  const uint8_t* bases = nullptr;
  const int64_t* ref_off = nullptr;  // [n_ref + 1]
  int32_t n_ref = 0;
  const uint64_t* known = nullptr;   // [(ref_off[n_ref] + 63) / 64]
};

constexpr size_t kBqCtxCells = (size_t)FCSBQ_NQ * FCSBQ_NCTX;  // per read group, (observations, errors) each
constexpr size_t kBqCycCells = (size_t)FCSBQ_NQ * FCSBQ_NCYC;

// Adds the batch's counts to ctx[n_rg][94][16][2] and cyc[n_rg][94][1000][2].
// Throws failedCommand, with nothing added, on a field out of range, a counted
// record of more than 500 kept bases or an aligned base beyond its contig.
// threads > 1: slices of the batch are counted into private tables and summed.
void bqsr_count_host(const BqRefView& ref, const fcsbq_batch& b, int32_t n_rg, int64_t* ctx, int64_t* cyc, int threads = 1);

// GATK's empirical quality of (observations, errors) under a prior quality.
double bqsr_emp_q(int64_t obs, int64_t err, double prior);

struct BqTables {
  int32_t n_rg = 0;
  std::vector<double> base, dctx, dcyc;  // [n_rg][94], [n_rg][94][16], [n_rg][94][1000]
};
BqTables bqsr_finalize(int32_t n_rg, const int64_t* ctx, const int64_t* cyc);

// The new qualities of the whole batch in its layout (records without a read
// group or qualities are copied).  Throws failedCommand, with nothing written,
// on a recalibrated record of more than 500 bases.
void bqsr_apply_host(const fcsbq_batch& b, const BqTables& t, uint8_t* out_qual, int threads = 1);

// GATKReport v1.1 text of the tables; names[n_rg] label the read groups.
std::string bqsr_report_text(int32_t n_rg, const int64_t* ctx, const int64_t* cyc, const std::vector<std::string>& names);
// The tables of a report (RecalTable1 is derived from RecalTable2's cycle rows
// and checked against it); a read group not in `names` throws formatError.
void bqsr_report_parse(const std::string& text, const std::vector<std::string>& names, std::vector<int64_t>& ctx,
                       std::vector<int64_t>& cyc);

}  // namespace fcsg
