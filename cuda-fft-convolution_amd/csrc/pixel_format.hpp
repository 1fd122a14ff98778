// pixel_format.hpp -- typed image pixels (fftconv_plan_set_images_typed): uint8 / uint16 / fp16 / bf16 elements whose value is
// their EXACT fp32 conversion -- no implied gain.  The conversions, the pixel types the kernel bodies are templates over and
// the loads of one element and of a pair of rows.  Written once, compiled twice like every header here: by hipcc into the
// kernels and by the host compiler into tests/pixel_format_host.
//
// A pixel TYPE is what a body is instantiated over: float (the fp32 text of every body, untouched), Pixel8 (one-byte elements:
// uint8) and Pixel16 (two-byte elements; WHICH of uint16 / fp16 / bf16 is PixelLoad::format, a uniform of the launch, as the
// fp16 / bf16 choice of the 16-bit output kernels is).
#pragma once
#include <cstdint>
#include <cstring>

#include "fc_common.hpp"

namespace fc {

// (the values of FFTCONV_PIXEL_* in include/fftconv.h)
constexpr int FC_PIXEL_F32 = 0, FC_PIXEL_U8 = 1, FC_PIXEL_U16 = 2, FC_PIXEL_F16 = 3, FC_PIXEL_BF16 = 4;
constexpr bool fc_pixel_format_ok(long f) { return f >= FC_PIXEL_F32 && f <= FC_PIXEL_BF16; }
constexpr size_t fc_pixel_elem_bytes(int format) { return format == FC_PIXEL_F32 ? 4 : format == FC_PIXEL_U8 ? 1 : 2; }

struct Pixel8 {};
struct Pixel16 {};
template <class Px> struct PixelElem { using type = float; };
template <> struct PixelElem<Pixel8> { using type = uint8_t; };
template <> struct PixelElem<Pixel16> { using type = uint16_t; };
template <class Px> using pixel_elem_t = typename PixelElem<Px>::type;

// What a typed launch knows about its pixels beyond their size, both uniform over the launch: the format (FC_PIXEL_*), and
// whether rows 2n, 2n + 1 of a column may come in ONE load (pixel_pair_load_ok).  The fp32 bodies never read it.
struct PixelLoad {
    int format = FC_PIXEL_F32;
    int wide = 0;
};

// A load is never wider than the address is known to be aligned (the rule of the output kernel's rectangle store): rows 2n and
// 2n + 1 of a column are one load of twice the element size only where the byte offset of EVERY such pair is a multiple of
// that -- the base address, the column pitch and the plane stride all even in elements.  Decided once per launch.
inline bool pixel_pair_load_ok(uintptr_t base_address, long col_pitch, size_t plane_stride, size_t elem_bytes) {
    if (elem_bytes != 1 && elem_bytes != 2) return false;      // (fp32 pixels keep their element loads)
    return base_address % (2 * elem_bytes) == 0 && col_pitch % 2 == 0 && plane_stride % 2 == 0;
}

// IEEE binary16 bits -> fp32, exact; subnormals kept.  Device: the hardware convert.
FC_HD float fc_f16_to_f32(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    _Float16 v;
    __builtin_memcpy(&v, &h, 2);
    return (float)v;
#else
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t u;
    if (e == 0x1fu) u = sign | 0x7f800000u | (m << 13);                 // inf / NaN (payload kept)
    else if (e != 0) u = sign | ((e + 112u) << 23) | (m << 13);
    else if (m == 0) u = sign;
    else {                                                             // subnormal: m * 2^-24, normal in fp32
        int s = 0;
        uint32_t mm = m;
        while (!(mm & 0x400u)) { mm <<= 1; s++; }
        u = sign | ((uint32_t)(113 - s) << 23) | ((mm & 0x3ffu) << 13);
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}
// bfloat16 bits -> fp32: the upper half of the word
FC_HD float fc_bf16_to_f32(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_memcpy(&f, &u, 4);
#else
    memcpy(&f, &u, 4);
#endif
    return f;
}

// the value of one element
FC_HD float pixel_value(float e, const PixelLoad&) { return e; }
FC_HD float pixel_value(uint8_t e, const PixelLoad&) { return (float)e; }
FC_HD float pixel_value(uint16_t e, const PixelLoad& px) {
    if (px.format == FC_PIXEL_F16) return fc_f16_to_f32(e);
    if (px.format == FC_PIXEL_BF16) return fc_bf16_to_f32(e);
    return (float)(uint32_t)e;
}

// rows r, r + 1 of a column in one load of twice the element size (little endian: the lower address in the low half); only
// where PixelLoad::wide says every pair is aligned for it
FC_HD void pixel_pair(const uint8_t* at, const PixelLoad& px, float& x0, float& x1) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t w = *reinterpret_cast<const uint16_t*>(at);
#else
    uint16_t w16;
    memcpy(&w16, at, 2);
    const uint32_t w = w16;
#endif
    x0 = pixel_value((uint8_t)(w & 0xffu), px);
    x1 = pixel_value((uint8_t)(w >> 8), px);
}
FC_HD void pixel_pair(const uint16_t* at, const PixelLoad& px, float& x0, float& x1) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t w = *reinterpret_cast<const uint32_t*>(at);
#else
    uint32_t w;
    memcpy(&w, at, 4);
#endif
    x0 = pixel_value((uint16_t)(w & 0xffffu), px);
    x1 = pixel_value((uint16_t)(w >> 16), px);
}

}  // namespace fc
