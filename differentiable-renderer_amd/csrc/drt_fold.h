// drt_fold.h -- the draw drt_rng_combine(h, key) (include/drt_hip.h: the definition) with the first step of its hash round
// taken out of the lanes' work.  drt_mix32 begins with x ^= x >> 16, which is linear over GF(2):
//     (h ^ key) ^ ((h ^ key) >> 16)  =  (h ^ (h >> 16)) ^ (key ^ (key >> 16))
// In the lockstep kernel h = h(n) is the same for every lane of a wave (the scalar unit computes it, and now its fold) and key is the
// same for every draw of a sample (folded once, behind the camera), so a draw starts with ONE exclusive-or where it had two -- the
// second a half-rate sub-dword select (v_xor_b32_sdwa ... WORD_1).  Integer arithmetic only: every draw keeps all 31 bits.
// Host + device: tests/cpp/fold_kat.cpp holds combine_folded(fold16(h), fold16(k)) against drt_rng_combine(h, k).
#pragma once

#if !defined(__HIPCC_RTC__)
#include <stdint.h>
#endif

#if defined(__HIPCC__)
#define DRT_FOLD_HD __host__ __device__ inline
#else
#define DRT_FOLD_HD inline
#endif

DRT_FOLD_HD uint32_t fold16(uint32_t x) { return x ^ (x >> 16); }

// drt_mix32's remaining steps on the folded halves, then the draw's >> 1
DRT_FOLD_HD uint32_t combine_folded(uint32_t hf, uint32_t kf)
{
    uint32_t x = hf ^ kf;
    x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x >> 1;
}
