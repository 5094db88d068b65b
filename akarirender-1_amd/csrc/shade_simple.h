// shade_simple.h — which shading build of the persistent path kernels a committed scene may run, decided on
// the device tables commit_scene() uploads and not on the scene's description.  The simple build
// (kernels.hip shade_hit_tab<.., SIMPLE = true>) reads every material channel and every light's emission as
// the record's constant, runs no Mix selection and fixes the closure to Diffuse once the Emissive case has
// returned; it is the general build with the branches a simple scene never takes folded away, so it may run
// only where the tables rule those branches out.  Plain C++, no HIP header: capi.hip's commit_scene() uses
// both functions, tests/cpp/shade_simple_check.cpp exercises them on hand-made tables.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/akr_hip.h"

namespace akr {

// A material channel's texture node as the device record holds it (MatDev's colour / roughness / fraction,
// LightDev's emission): a constant node becomes the record's value and leaves `img` at -1
// (Texture::evaluate of a ConstantTexture is its value); an image node leaves the value alone and names
// itself in `img`.  An index outside the texture list is a channel the material's type does not use.
template <class Tex>
inline void resolve_channel(const Tex *texs, size_t n_texs, int32_t ti, float *val, int n, int32_t &img) {
    if (ti < 0 || (size_t)ti >= n_texs) return;
    if (texs[ti].type == AKR_TEX_IMAGE) {
        img = ti;
        return;
    }
    for (int c = 0; c < n; c++) val[c] = texs[ti].value[c];
}

// A material's device record (MatDev: zeroed by the caller): the type's channels resolved, every other
// *_img left at -1.
template <class Mat, class Tex>
inline void resolve_material(const akr_material &x, const Tex *texs, size_t n_texs, Mat &d) {
    d.type = x.type;
    d.double_sided = x.double_sided;
    d.first = x.first;
    d.second = x.second;
    d.color_img = d.rough_img = d.frac_img = -1;
    if (x.type == AKR_MAT_DIFFUSE || x.type == AKR_MAT_EMISSIVE || x.type == AKR_MAT_GLOSSY ||
        x.type == AKR_MAT_MIRROR || x.type == AKR_MAT_GLASS)
        resolve_channel(texs, n_texs, x.color, d.color, 3, d.color_img);
    // Glass: `rough` holds the index of refraction (a constant: commit_scene() refuses an image)
    if (x.type == AKR_MAT_GLOSSY || x.type == AKR_MAT_GLASS)
        resolve_channel(texs, n_texs, x.roughness, &d.rough, 1, d.rough_img);
    if (x.type == AKR_MAT_MIX) resolve_channel(texs, n_texs, x.fraction, &d.frac, 1, d.frac_img);
}

// A light's emission (LightDev::color_img, Le) from its Emissive material's colour node `ti` (a valid index)
template <class Light, class Tex>
inline void resolve_emission(const Tex *texs, size_t n_texs, int32_t ti, Light &x) {
    x.color_img = -1;
    x.Le[0] = x.Le[1] = x.Le[2] = 0.0f;
    resolve_channel(texs, n_texs, ti, x.Le, 3, x.color_img);
}

// True when the tables hold nothing the simple shading build leaves out: every material Diffuse or
// Emissive, no channel of any material an image (every *_img < 0), and no light's emission an image.
// A material no triangle uses counts: a Mix may reach any record, and the rule stays one pass over the
// tables.  Mat has type, color_img, rough_img, frac_img; Light has color_img (akr_device.h MatDev, LightDev).
template <class Mat, class Light>
inline bool shade_tables_simple(const Mat *mats, size_t n_mats, const Light *lights, size_t n_lights) {
    for (size_t m = 0; m < n_mats; m++) {
        const Mat &x = mats[m];
        if (x.type != AKR_MAT_DIFFUSE && x.type != AKR_MAT_EMISSIVE) return false;
        if (x.color_img >= 0 || x.rough_img >= 0 || x.frac_img >= 0) return false;
    }
    for (size_t l = 0; l < n_lights; l++)
        if (lights[l].color_img >= 0) return false;
    return true;
}

}  // namespace akr
