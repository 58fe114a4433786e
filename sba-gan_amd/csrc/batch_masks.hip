// The two masks of a training batch from integers already on the device (sba_batch_masks in sbagan_hip.h;
// sbagan/static_batch.py): the padding mask of the captions and the same-class mask of the DAMSM losses.
//
// One grid-stride pass over B * L + B * B bytes: plain loads, plain byte stores, no atomics, no LDS.  Deterministic and
// free of host state, so the launch can be recorded in front of the training step.
#include "common.h"

namespace {

constexpr int BM_THREADS = 256;
constexpr int BM_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(BM_THREADS) void batch_masks_kernel(
    const int64_t* __restrict__ captions, const int64_t* __restrict__ class_ids, uint8_t* __restrict__ word_mask,
    uint8_t* __restrict__ class_mask, int B, int L) {
    const int64_t nw = (int64_t)B * L, n = nw + (int64_t)B * B;
    const int64_t stride = (int64_t)gridDim.x * BM_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * BM_THREADS + threadIdx.x; e < n; e += stride) {
        if (e < nw) {
            word_mask[e] = captions[e] == 0 ? 1 : 0;
        } else {
            const int64_t q = e - nw;
            const int i = (int)(q / B), j = (int)(q % B);
            class_mask[q] = (j != i && class_ids[j] == class_ids[i]) ? 1 : 0;   // 64-bit compare
        }
    }
}

}  // namespace

extern "C" int sba_batch_masks(const int64_t* captions, const int64_t* class_ids, uint8_t* word_mask,
                               uint8_t* class_mask, int B, int L, void* stream) {
    if (!captions || !class_ids || !word_mask || !class_mask) return SBA_E_ARG;
    if (B < 1 || L < 1 || B > 65535 || L > 65535) return SBA_E_ARG;
    const int64_t n = (int64_t)B * L + (int64_t)B * B;
    int blocks = cdiv(n, BM_THREADS);
    if (blocks > BM_MAX_BLOCKS) blocks = BM_MAX_BLOCKS;
    SBA_LAUNCH(batch_masks_kernel, dim3(blocks), dim3(BM_THREADS), 0, (hipStream_t)stream, captions, class_ids,
               word_mask, class_mask, B, L);
    return SBA_CHECK_LAUNCH();
}
