// rs_pbrt_amd — the material bookkeeping of rspt_scene_create as one host step: the two lobe sets of material_assembly.h, what the
// scene can put in front of the shade stage (shade_features, shade_classes), and the per-material texture slots.  Host only.
// prepare_scene() runs it between the refusals of scene_validate.h, in the order the first error of a faulty scene depends on.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "material_assembly.h"
#include "scene_validate.h"

namespace rspt {
namespace scene {

// [0]: allow_multiple_lobes — path, volpath, ao; [1]: not — directlighting, whitted
struct SceneMaterials {
    std::vector<rspt_material> mats[2];
    std::vector<rspt_bxdf> bxdfs[2];            // texture ids until number_texture_slots, then slot numbers (1 + slot)
    std::vector<rspt_mat::DynMaterial> dyn[2];  // [material] when the variant has a dynamic material, else empty
    std::vector<uint8_t> is_dyn[2];
    std::vector<uint32_t> slots[2];             // [material][RSPT_TEX_SLOTS]: texture | RSPT_SLOT_* of every slot, 0xffffffff = unused
    std::vector<uint8_t> mflags[2];             // RSPT_MAT_* per material
    bool textured[2] = {false, false};          // some material of the set has a flag set
    uint32_t shade_features = 0;                // SF_* (dev_bsdf.h)
    uint32_t shade_classes = 0;                 // distinct lobe-list shapes among the materials
};

// materials: Material::compute_scattering_functions restated on the host (material_assembly.h), once per allow_multiple_lobes
inline Error assemble_materials(const rspt_scene_desc* d, const SceneFacts& f, SceneMaterials* out) {
    SceneMaterials& sm = *out;
    for (int v = 0; v < 2; v++) {
        rspt_mat::Assembler as(d, v == 0);
        rspt_mat::Lobes lb;
        sm.mats[v].resize(d->n_materials);
        sm.is_dyn[v].assign(d->n_materials, 0);
        for (uint32_t i = 0; i < d->n_materials; i++) {
            if (Error e = as.assemble(i, &lb)) return e;
            lb.mat.first_bxdf = (uint32_t)sm.bxdfs[v].size();
            sm.mats[v][i] = lb.mat;
            sm.bxdfs[v].insert(sm.bxdfs[v].end(), lb.lobes.begin(), lb.lobes.end());
            if (lb.dynamic) {
                if (sm.dyn[v].empty()) sm.dyn[v].resize(d->n_materials);
                sm.dyn[v][i] = lb.dyn;
                sm.is_dyn[v][i] = 1;
            }
        }
    }
    uint32_t shade_features = 0;
    for (int v = 0; v < 2; v++)
        for (const rspt_bxdf& b : sm.bxdfs[v]) {
            shade_features |= RSPT_SF_LOBE(b.type);
            if (b.fresnel == RSPT_FRESNEL_CONDUCTOR) shade_features |= SF_CONDUCTOR;
            if (b.has_sc) shade_features |= SF_SC;
            if (b.tex_r || b.tex_t || b.tex_ax || b.tex_ay) shade_features |= SF_TEX;
        }
    for (int v = 0; v < 2; v++)
        for (const rspt_material& m : sm.mats[v]) if (m.bump_tex) shade_features |= SF_TEX;
    {   // materials whose lobe lists have the same types in the same order (and the same textured-ness) cost a wave the same
        std::vector<std::string> seen;
        for (uint32_t i = 0; i < d->n_materials; i++) {
            const rspt_material& m = sm.mats[0][i];
            std::string sig = sm.is_dyn[0][i] ? "dyn" : "";
            for (uint32_t l = 0; l < m.n_bxdfs; l++) {
                const rspt_bxdf& b = sm.bxdfs[0][m.first_bxdf + l];
                sig += (char)('a' + b.type); sig += (char)('0' + b.fresnel); sig += (b.tex_r || b.tex_t || b.tex_ax || b.tex_ay) ? 't' : 'c';
            }
            if (m.bump_tex) sig += 'B';
            if (std::find(seen.begin(), seen.end(), sig) == seen.end()) seen.push_back(sig);
        }
        sm.shade_classes = (uint32_t)seen.size();
    }
    if (!sm.dyn[0].empty() || !sm.dyn[1].empty())  // a list built per hit may hold any lobe its material kind can push
        shade_features |= SF_DYNAMIC | SF_TEX | 0x3feu | SF_CONDUCTOR | SF_SC;
    for (uint32_t i = 0; i < d->n_lights; i++) {
        const uint32_t k = d->lights[i].kind;
        shade_features |= k == RSPT_LIGHT_DIFFUSE_AREA ? SF_L_AREA : (k == RSPT_LIGHT_POINT ? SF_L_POINT : (k == RSPT_LIGHT_SPOT ? SF_L_SPOT : (k == RSPT_LIGHT_DISTANT ? SF_L_DISTANT : (k == RSPT_LIGHT_INFINITE ? SF_L_INFINITE : SF_L_MAP))));
    }
    for (uint32_t i = 0; i < d->n_meshes; i++)
        if (d->meshes[i].has_n || d->meshes[i].has_s || d->meshes[i].has_uv) shade_features |= SF_VERTEX;
    if (f.instanced) shade_features |= SF_INST;
    if (f.has_null || (f.instanced && d->instancing_mode == RSPT_INSTANCING_REFERENCE)) shade_features |= SF_NULL;
    sm.shade_features = shade_features;
    return Error{};
}

// lobes: texture ids become per-material slot numbers (1 + slot) for k_texture / k_shade
inline Error number_texture_slots(const rspt_scene_desc* d, SceneMaterials* sm) {
    for (int v = 0; v < 2; v++) {
        std::vector<rspt_bxdf>& bx = sm->bxdfs[v];
        std::vector<uint32_t>& slots = sm->slots[v];
        std::vector<uint8_t>& mflags = sm->mflags[v];
        slots.assign((size_t)d->n_materials * RSPT_TEX_SLOTS, 0xffffffffu);
        mflags.assign(d->n_materials, 0);
        bool any_v = false;
        for (uint32_t m = 0; m < d->n_materials; m++) {
            const rspt_material& mat = sm->mats[v][m];
            uint32_t* sl = slots.data() + (size_t)m * RSPT_TEX_SLOTS;
            uint32_t n_sl = 0;
            bool full = false;
            auto slot_of = [&](uint32_t tex_plus_1, uint32_t flags) -> uint32_t {
                const uint32_t desc = (tex_plus_1 - 1u) | flags;
                for (uint32_t k = 0; k < n_sl; k++) if (sl[k] == desc) return k + 1u;
                if (n_sl == RSPT_TEX_SLOTS) { full = true; return 1u; }
                sl[n_sl++] = desc;
                return n_sl;
            };
            for (uint32_t l = 0; l < mat.n_bxdfs; l++) {
                rspt_bxdf& b = bx[mat.first_bxdf + l];
                const uint32_t nd = (b.remap & RSPT_LOBE_NODIFF) ? RSPT_SLOT_NODIFF : 0u;  // the m2 side of a mix (mixmat.rs:58-69)
                const uint32_t aflags = RSPT_SLOT_ALPHA | ((b.remap & RSPT_LOBE_REMAP) ? RSPT_SLOT_REMAP : 0u) | nd;
                if (b.tex_r) { b.tex_r = slot_of(b.tex_r, nd); mflags[m] |= RSPT_MAT_TEXTURED; }
                if (b.tex_t) { b.tex_t = slot_of(b.tex_t, nd); mflags[m] |= RSPT_MAT_TEXTURED; }
                if (b.tex_ax) { b.tex_ax = slot_of(b.tex_ax, aflags); mflags[m] |= RSPT_MAT_TEXTURED; }
                if (b.tex_ay) { b.tex_ay = slot_of(b.tex_ay, aflags); mflags[m] |= RSPT_MAT_TEXTURED; }
            }
            if (full) return refuse(RSPT_E_UNSUPPORTED, "material %u binds more than %d distinct textures", m, RSPT_TEX_SLOTS);
            if (sm->is_dyn[v][m]) mflags[m] |= RSPT_MAT_DYNAMIC | RSPT_MAT_TEXTURED;
            if (mat.bump_tex) mflags[m] |= RSPT_MAT_BUMP;
            any_v |= mflags[m] != 0;
        }
        sm->textured[v] = any_v;
    }
    return Error{};
}

// Everything rspt_scene_create does before it touches the device, in the order a scene with several faults reports them: the refusals
// up to the texture graph, the material assembly, the envmaps and the BVH, the slot numbering, the moving instances.
inline Error prepare_scene(const rspt_scene_desc* d, SceneFacts* facts, SceneMaterials* sm) {
    Error e;
    if ((e = validate_scene(d, facts)) || (e = assemble_materials(d, *facts, sm)) || (e = validate_envmaps_and_bvh(d, *facts)) ||
        (e = number_texture_slots(d, sm)) || (e = validate_animated_instances(d)))
        return e;
    return Error{};
}

}  // namespace scene
}  // namespace rspt
