// attention_wide_shape.h -- the constants of the LDS-staged attention kernels of head dims 72, 80, .., 128 (attention_wide.hip, attention_packed_wide.hip),
// which say what the names mean: P pieces of 16 bytes in a head's row slice, 64-key chunks of unpadded rows, a K image and a V image per chunk buffer,
// two buffers, and the rotation of K's pieces inside their row that makes a fragment read conflict-free.
#pragma once

namespace vitx {

template <int DH>
struct WideShape {
    static constexpr int P = DH / 8, NK2 = DH <= 96 ? 3 : 4, NDV = (DH + 15) / 16, ROWB = DH * 2;
    static constexpr int G = (P & -P) > 16 ? 16 : (P & -P);                    // gcd(P, 16)
    static constexpr int CK = 64, KBYTES = CK * ROWB, BUF = 2 * KBYTES;         // a chunk buffer: K image, then V image
    static constexpr int LDS = 2 * BUF + (DH % 16 ? 16 : 0);
    static constexpr int WAVES = 160 * 1024 / LDS > 4 ? 4 : 160 * 1024 / LDS;   // workgroups (= waves per SIMD) the LDS lets a CU hold
    static __device__ __forceinline__ int rot(int r) { return ((r & 15) * G) >> 4; }
};

}  // namespace vitx
