// encode_crc.h -- the fused encode + CRC-32 launch (encode_crc_kernels.hip):
// one pass over a set that forms every stripe's parity cells and leaves the
// CRC-32 tile remainders of all its cells, data and parity, for
// crc32_finish_kernel (crc32.h). Shared by the kernels and the plans
// (redset_hip.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "codec_kernels.h"
#include "crc32.h"

namespace redset_hip {

// One launch over `njobs` stripes of `nin` data cells and `nout` parity cells
// of `nbytes` bytes each, every cell 16-B aligned. Block (job, tile) writes
// rem[slot[job * (nin + nout) + c] * tiles + tile] for cell c of the job
// (inputs, then outputs): what crc32_tiles_kernel writes for that tile of the
// range (cell, nbytes). `finish` is the launch of crc32_finish_kernel over the
// same `rem`, one range per cell: finish.tile_base[s] = s * tiles.
struct EncodeCrcLaunch {
  const GfJob* jobs;       // device; XOR stripes use in[] and out[0] only
  const int* slot;         // device: njobs * (nin + nout) range numbers
  const unsigned* xpow;    // device: kCrcLanes powers of x, one per thread (encode_crc_xpow)
  const unsigned* tables;  // device: crc_device_tables()
  unsigned* rem;           // device: one remainder per (range, tile)
  int njobs, nin, nout;
  int xor_only;            // 1: parity = XOR of the inputs, no GF tables
  int tiles;               // crc_tiles of a cell (0 for cells under kCrcSeg bytes)
  size_t nbytes;
  CrcLaunch finish;
};

// xpow[t] for thread t of the block: x^(8 n), n = the bytes between the end
// of that thread's last vector of a tile and the tile's end
void encode_crc_xpow(unsigned* xpow);
// both kernels of one execute on `stream`; returns hipError_t as int
int launch_encode_crc(const EncodeCrcLaunch& L, void* stream);

}  // namespace redset_hip
