// verify_crc.h -- the fused verify + CRC-32 launch (verify_crc_kernels.hip):
// one pass over a set that checks every stripe's stored parity against its
// stored data, as the verify plans' check kernels do (codec_kernels.h), and
// leaves the CRC-32 tile remainders of all its cells, data and parity, for
// crc32_finish_kernel (crc32.h). No cell is written. Shared by the kernels
// and the plans (redset_hip.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "codec_kernels.h"
#include "crc32.h"

namespace redset_hip {

// One launch over `njobs` stripes of `nin` data cells (jobs[k].in) and `nout`
// STORED parity cells (jobs[k].out, only read; coef as the encode's) of
// `nbytes` bytes each, every cell 16-B aligned. Job k reports to rows
// [k * nout, + nout) of `report` as a check launch does (GfCheckLaunch:
// report[row] counts the differing bytes of that parity row, report[
// report_rows + row] holds the smallest differing cell offset, ~0 if none);
// XOR stripes have one row, the XOR of all nin + 1 cells. Block (job, tile)
// writes rem[slot[job * (nin + nout) + c] * tiles + tile] for cell c of the
// job (inputs, then outputs) from the bytes it LOADED: what crc32_tiles_kernel
// writes for that tile of the range (cell, nbytes). `finish` is the launch of
// crc32_finish_kernel over the same `rem`, one range per cell.
struct VerifyCrcLaunch {
  const GfJob* jobs;           // device; XOR stripes use in[] and out[0] only
  const int* slot;             // device: njobs * (nin + nout) range numbers
  const unsigned* xpow;        // device: kCrcLanes powers of x, one per thread (encode_crc_xpow)
  const unsigned* tables;      // device: crc_device_tables()
  unsigned* rem;               // device: one remainder per (range, tile)
  unsigned long long* report;  // device: report_rows counts, then report_rows first offsets
  int report_rows;             // njobs * nout
  int njobs, nin, nout;
  int xor_only;                // 1: the syndrome is the XOR of the cells, no GF tables
  int tiles;                   // crc_tiles of a cell (0 for cells under kCrcSeg bytes)
  size_t nbytes;
  CrcLaunch finish;
};

// the three kernels of one execute on `stream` -- the report's reset (one
// block), the fused kernel, the CRC finish; returns hipError_t as int
int launch_verify_crc(const VerifyCrcLaunch& L, void* stream);

}  // namespace redset_hip
