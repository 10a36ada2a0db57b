// Per-pixel arithmetic of torchvision 0.8.2's PIL ColorJitter, restated from Pillow's C sources operation by operation
// (libImaging/Blend.c ImagingBlend, Convert.c rgb2l / rgb2hsv_row / hsv2rgb, ImageEnhance.Brightness / Contrast /
// Color).  Every intermediate keeps Pillow's type -- float where Pillow holds a float, double where C's usual
// arithmetic conversions promote (a double literal in the expression) -- so that the bytes are Pillow's.  The file is
// built with -ffp-contract=off.  Plain C++ behind PD_HD, so the same text runs in the kernels of color.hip and in a
// host compiler.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PD_HD __host__ __device__ __forceinline__
#else
#define PD_HD inline
#endif

namespace pdcolor {

enum { kNone = 0, kBrightness = 1, kContrast = 2, kSaturation = 3, kHue = 4 };

// One params row, decoded: what every pixel of a sample applies, in order.
struct Chain {
    int code[4];
    float alpha[4];    // blend factor as Pillow's float
    int shift[4];      // hue: (uint8)(int)(value * 255.0)
    int contrast_at;   // index of the contrast operation, 4 when the row has none
};

// codes other than 1..4 are 0; a row holds each operation once (ColorJitter's rows do): a second contrast would need a
// second mean over the whole sample, so only the first is honoured and a repeated one behaves as 0
PD_HD Chain decode_row(const double* row) {
    Chain ch;
    ch.contrast_at = 4;
    for (int k = 0; k < 4; ++k) {
        const double c = row[2 * k], v = row[2 * k + 1];
        int code = c == 1.0 ? kBrightness : c == 2.0 ? kContrast : c == 3.0 ? kSaturation : c == 4.0 ? kHue : kNone;
        if (code == kContrast) {
            if (ch.contrast_at < 4) code = kNone;
            else ch.contrast_at = k;
        }
        ch.code[k] = code;
        ch.alpha[k] = (float)v;
        ch.shift[k] = code == kHue ? ((int)(v * 255.0) & 0xff) : 0;
    }
    return ch;
}

PD_HD int clip8i(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ImagingConvert rgb2l
PD_HD int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// ImagingBlend(in1 = degenerate, in2 = image, alpha): interpolation truncates, extrapolation clips first
PD_HD int blend(int d, int x, float a) {
    const float t = (float)d + a * (float)(x - d);
    if (a >= 0.0f && a <= 1.0f) return (int)(uint8_t)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)(uint8_t)t);
}

PD_HD void rgb2hsv(int r, int g, int b, int& uh, int& us, int& uv) {
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    uv = maxc;
    if (minc == maxc) {
        uh = us = 0;
        return;
    }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double t = (double)h / 6.0 + 1.0;        // in (0.8, 1.9): fmod(t, 1.0) is t minus its integer part, exactly
    h = (float)(t - floor(t));
    uh = clip8i((int)((double)h * 255.0));
    us = clip8i((int)((double)s * 255.0));
}

PD_HD void hsv2rgb(int h, int s, int v, int& r, int& g, int& b) {
    if (s == 0) {
        r = g = b = v;
        return;
    }
    const double hf = (double)(float)h * 6.0 / 255.0;
    const int i = (int)floor(hf);
    const float f = (float)(hf - (double)(float)i);
    const float fs = (float)((double)(float)s / 255.0);
    const double vd = (double)(float)v;
    const int p = clip8i((int)round(vd * (1.0 - (double)fs)));
    const int q = clip8i((int)round(vd * (1.0 - (double)(fs * f))));
    const int t = clip8i((int)round(vd * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// operations [k0, k1) of the chain on one pixel; mean = the contrast degenerate of the pixel's sample
PD_HD void apply_ops(const Chain& ch, int k0, int k1, int mean, int& r, int& g, int& b) {
    for (int k = k0; k < k1; ++k) {
        const float a = ch.alpha[k];
        switch (ch.code[k]) {
            case kBrightness: r = blend(0, r, a); g = blend(0, g, a); b = blend(0, b, a); break;
            case kContrast: r = blend(mean, r, a); g = blend(mean, g, a); b = blend(mean, b, a); break;
            case kSaturation: {
                const int l = luma(r, g, b);
                r = blend(l, r, a); g = blend(l, g, a); b = blend(l, b, a);
                break;
            }
            case kHue: {
                int h, s, v;
                rgb2hsv(r, g, b, h, s, v);
                hsv2rgb((h + ch.shift[k]) & 0xff, s, v, r, g, b);
                break;
            }
            default: break;
        }
    }
}

// ImageEnhance.Contrast: int(ImageStat.Stat(L).mean[0] + 0.5) from the exact integer sum of L over the sample
PD_HD int contrast_mean(unsigned long long sum, long count) { return (int)((double)sum / (double)count + 0.5); }

}  // namespace pdcolor
