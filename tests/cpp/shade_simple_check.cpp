// Drives csrc/shade_simple.h for tests/test_shade_simple_host.py.  Each input line describes a scene's
// texture, material and light lists as commit_scene() sees them, as space-separated tokens:
//   t:c            a constant texture node                 t:i            an image texture node
//   m:d:<T>        Diffuse, colour node T                  m:e:<T>        Emissive, colour node T
//   m:g:<T>:<R>    Glossy, colour T, roughness R           m:x:<F>:<A>:<B> Mix, fraction node F of materials A, B
//   l:<M>          a light on a triangle of (Emissive) material M
//   M:<type>:<color_img>:<rough_img>:<frac_img>            a material record as it stands
//   L:<color_img>                                          a light record as it stands
// The records are resolved as commit_scene() resolves them (resolve_material, resolve_emission) and the
// reply is one line: "simple=<0|1> mats=<color_img>/<rough_img>/<frac_img>,... lights=<color_img>,..."
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "shade_simple.h"

// the fields of akr_device.h's MatDev and LightDev that the header touches (those need HIP's float4)
struct Mat {
    int32_t type, double_sided, first, second;
    float color[3];
    int32_t color_img;
    float rough;
    int32_t rough_img;
    float frac;
    int32_t frac_img;
};
struct Light {
    int32_t color_img;
    float Le[3];
};

static std::vector<int> fields(const std::string &tok) {  // the integers behind the two leading letters
    std::vector<int> v;
    std::istringstream in(tok.size() > 4 ? tok.substr(4) : std::string());
    std::string f;
    while (std::getline(in, f, ':')) v.push_back(std::stoi(f));
    return v;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::vector<akr_texture> texs;
        std::vector<akr_material> mats;
        std::vector<int> light_mat;
        std::istringstream in(line);
        std::string tok;
        while (in >> tok) {
            if (tok == "t:c" || tok == "t:i") {
                akr_texture t{};
                t.type = tok == "t:i" ? AKR_TEX_IMAGE : AKR_TEX_CONSTANT;
                t.value[0] = t.value[1] = t.value[2] = 0.5f;
                texs.push_back(t);
            } else if (tok.rfind("m:", 0) == 0 && tok.size() >= 3) {
                const std::vector<int> f = fields(tok);
                akr_material m{};
                m.color = m.roughness = m.fraction = m.first = m.second = -1;
                const char k = tok[2];
                if (k == 'd' || k == 'e') {
                    m.type = k == 'd' ? AKR_MAT_DIFFUSE : AKR_MAT_EMISSIVE;
                    m.color = f.at(0);
                } else if (k == 'g') {
                    m.type = AKR_MAT_GLOSSY;
                    m.color = f.at(0);
                    m.roughness = f.at(1);
                } else {
                    m.type = AKR_MAT_MIX;
                    m.fraction = f.at(0);
                    m.first = f.at(1);
                    m.second = f.at(2);
                }
                mats.push_back(m);
            } else if (tok.rfind("l:", 0) == 0) {
                light_mat.push_back(std::stoi(tok.substr(2)));
            }
        }
        std::vector<Mat> md(mats.size());
        for (size_t i = 0; i < mats.size(); i++) {
            std::memset(&md[i], 0, sizeof(Mat));
            akr::resolve_material(mats[i], texs.data(), texs.size(), md[i]);
        }
        std::vector<Light> ld(light_mat.size());
        for (size_t i = 0; i < ld.size(); i++)
            akr::resolve_emission(texs.data(), texs.size(), mats.at((size_t)light_mat[i]).color, ld[i]);
        // records given as they stand, behind the resolved ones
        std::istringstream raw(line);
        while (raw >> tok) {
            if (tok.rfind("M:", 0) == 0) {
                const std::vector<int> f = fields("M:_:" + tok.substr(2));
                Mat d{};
                d.type = f.at(0);
                d.color_img = f.at(1);
                d.rough_img = f.at(2);
                d.frac_img = f.at(3);
                md.push_back(d);
            } else if (tok.rfind("L:", 0) == 0) {
                Light l{};
                l.color_img = std::stoi(tok.substr(2));
                ld.push_back(l);
            }
        }
        std::printf("simple=%d mats=", akr::shade_tables_simple(md.data(), md.size(), ld.data(), ld.size()) ? 1 : 0);
        for (size_t i = 0; i < md.size(); i++)
            std::printf("%s%d/%d/%d", i ? "," : "", md[i].color_img, md[i].rough_img, md[i].frac_img);
        std::printf(" lights=");
        for (size_t i = 0; i < ld.size(); i++) std::printf("%s%d", i ? "," : "", ld[i].color_img);
        std::printf("\n");
    }
    return 0;
}
