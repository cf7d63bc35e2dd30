// batch_chunks.h -- how a launch of the two batch kernels (compat_batch.hip,
// alt_batch_kernel in alt_kernels.hip) cuts its n frames into chunks, as a
// function of plain numbers.  No HIP here (tests/test_batch_chunks_cpu.py
// compiles this header alone with g++): the wave slots the kernel has
// resident come in as a value.
#pragma once

#include <algorithm>
#include <cstdint>

namespace dips_sched {

struct BatchChunks {
    uint32_t chunk = 0;     // frames per chunk (the last one may hold fewer)
    uint64_t n_chunks = 0;  // chunk c holds frames [c * chunk, min((c + 1) * chunk, n))
};

// A wave walks one (tile, chunk) item with its per-pixel state in registers
// and every chunk after the first rebuilds that state from HBM, so: enough
// items to fill the resident wave slots, but at most ceil(n / 16) chunks
// (n = 17 gives chunks of 9 and 8), of equal length but for the last.
// n >= 1, n_tiles >= 1.
inline BatchChunks batch_chunk_plan(uint64_t n, uint64_t n_tiles, uint64_t resident) {
    uint64_t n_chunks = (resident + n_tiles - 1) / n_tiles;
    n_chunks = std::min<uint64_t>(n_chunks, (n + 15u) / 16u);
    n_chunks = std::max<uint64_t>(n_chunks, 1);
    BatchChunks p;
    p.chunk = (uint32_t)((n + n_chunks - 1) / n_chunks);
    p.n_chunks = (n + p.chunk - 1) / p.chunk;
    return p;
}

}  // namespace dips_sched
