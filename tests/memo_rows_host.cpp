// memo_rows_host.cpp — TEST INFRASTRUCTURE: k_memo_rows (ss_kernels.hpp; include/ss_hip.h "Pose memo on the column path")
// compiled for the host with tests/hostsim/hip_shim.h (hostsim.cpp included whole for the thread / block index globals), so
// tests/test_memo_rows_host.py can check every byte it moves - and every byte it must not touch - against numpy without a GPU.
// The kernel has no barrier and no shared memory: its 256 threads run one after the other, no fibers needed.
// Never part of the product.
#include "hostsim/hostsim.cpp"

#include <cstring>

// One launch as ss_memo_rows_f32 / ss_ctx_observe_sims_memo issue it: grid (chunks of the longest row, move, array).
// tab != 0: the moves ride in the kernel-argument table (<= kMemoTabMoves), else they are read through the pointer.
extern "C" int hs_memo_rows(float* const* out, float* const* pool, const int* row_floats, int n_io, const int* moves, int n_store,
                            int n_fetch, int tab) {
    const int n = n_store + n_fetch;
    if (n_io < 1 || n_io > ssk::kMemoArrays || n < 0 || (tab && n > ssk::kMemoTabMoves)) return -1;
    ssk::MemoRowsParams p;
    int longest = 1;
    for (int a = 0; a < ssk::kMemoArrays; ++a) {
        const int b = a < n_io ? a : 0;
        p.out[a] = out[b]; p.pool[a] = pool[b]; p.row_floats[a] = row_floats[b];
        if (row_floats[b] > longest) longest = row_floats[b];
    }
    p.moves = tab ? nullptr : moves;
    p.n_store = n_store;
    ssk::MoveTab<true> mt;
    std::memset(&mt, 0xff, sizeof mt);
    if (tab) std::memcpy(mt.mv, moves, sizeof(int) * 2 * (size_t)n);
    const unsigned gx = (unsigned)((longest + ssk::kMemoChunk - 1) / ssk::kMemoChunk);
    gridDim = dim3{gx, (unsigned)n, (unsigned)n_io};
    blockDim = dim3{256, 1, 1};
    for (unsigned z = 0; z < (unsigned)n_io; ++z)
        for (unsigned y = 0; y < (unsigned)n; ++y)
            for (unsigned x = 0; x < gx; ++x) {
                blockIdx = dim3{x, y, z};
                for (unsigned t = 0; t < 256; ++t) {
                    threadIdx = dim3{t, 0, 0};
                    if (tab) ssk::k_memo_rows<true>(p, mt);
                    else ssk::k_memo_rows<false>(p);
                }
            }
    return 0;
}
