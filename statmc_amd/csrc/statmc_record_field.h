// statmc_record_field.h -- one field of an interleaved record (statmc_record_layout, include/statmc.h) as a kernel requests it
// and as it folds it: what the records fold (statmc_records.hip) and the compact interleaved fold (statmc_compact.hip) share.
// Device code only; every definition is internal to the translation unit that includes it.
#pragma once

#include <hip/hip_runtime.h>

namespace statmc {

namespace {

// 4-byte aligned wide accesses: an RGB field is 12 B at any 4-byte aligned offset
typedef unsigned rec_uint3 __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned rec_uint2 __attribute__((ext_vector_type(2), aligned(4)));

// The loaded dwords of one record: what a batch holds between request and fold.  What is in flight stays RAW: a half is widened
// when its sample is folded, not when it is requested -- a conversion behind the load would wait for it there and nothing would
// run ahead.
template <int N>
struct RecRaw {
    unsigned r[N];
    __device__ __forceinline__ void pin() {      // walk_run's empty asm (trap 1 of DESIGN 4.1c)
#pragma unroll
        for (int i = 0; i < N; i++) asm("" : "+v"(r[i]));
    }
};

// every finite half is an fp32 value, subnormals included: one v_cvt_f32_f16
__device__ __forceinline__ float rec_half_to_float(unsigned bits16) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16); }

// One field of a record -- C elements -- as it is requested and as it is folded.
//   kFieldF32         C floats at a 4-byte aligned address: one dword, or one dwordx3
//   kFieldHalfElems   C halves at a 2-byte aligned address, element by element (the fold of one type)
//   kFieldHalfDwords  C halves as the dwords that hold them (the fused fold): load() is given the field's address rounded DOWN
//                     to 4 bytes, decode() the bit position of the first element in the first dword (0 or 16).  The record
//                     starts 4-byte aligned and the stride is a multiple of 4, so the dwords lie inside the record: three
//                     halves at offset o occupy [o, o + 6) and are read as [o & ~3, (o & ~3) + 8), one half as one dword.
enum { kFieldF32 = 0, kFieldHalfElems, kFieldHalfDwords };
template <int C, int F>
struct RecField {
    static constexpr int kRegs = F == kFieldHalfDwords ? (C == 3 ? 2 : 1) : C;
    static __device__ __forceinline__ void load(const char *__restrict__ at, unsigned *r) {
        if constexpr (F == kFieldHalfElems) {
            const unsigned short *h = reinterpret_cast<const unsigned short *>(at);
#pragma unroll
            for (int c = 0; c < C; c++) r[c] = h[c];
        } else if constexpr (kRegs == 3) {
            const rec_uint3 x = *reinterpret_cast<const rec_uint3 *>(at);
            r[0] = x.x;
            r[1] = x.y;
            r[2] = x.z;
        } else if constexpr (kRegs == 2) {
            const rec_uint2 x = *reinterpret_cast<const rec_uint2 *>(at);
            r[0] = x.x;
            r[1] = x.y;
        } else {
            r[0] = *reinterpret_cast<const unsigned *>(at);
        }
    }
    static __device__ __forceinline__ void decode(const unsigned *r, int shift, float *v) {
        if constexpr (F == kFieldF32) {
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = __uint_as_float(r[c]);
        } else if constexpr (F == kFieldHalfElems) {
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = rec_half_to_float(r[c]);
        } else if constexpr (C == 3) {
            const unsigned long long w = (((unsigned long long)r[1] << 32) | r[0]) >> shift;
            v[0] = rec_half_to_float((unsigned)w & 0xffffu);
            v[1] = rec_half_to_float((unsigned)(w >> 16) & 0xffffu);
            v[2] = rec_half_to_float((unsigned)(w >> 32) & 0xffffu);
        } else {
            v[0] = rec_half_to_float((r[0] >> shift) & 0xffffu);
        }
    }
};

}  // namespace

}  // namespace statmc
