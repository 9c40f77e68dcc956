// rs_pbrt_amd — what rspt_scene_create refuses: every index, range and number of an rspt_scene_desc is checked here, on the host, before
// anything is allocated (a bad scene must not fault the GPU).  Host only: no HIP call, no global state, so tests/scene_host_main.hip runs
// every refusal on a machine without a GPU.
//
// Order is part of the contract (a scene with several faults reports the first): validate_scene, then the material assembly
// (scene_materials.h assemble_materials), then validate_envmaps_and_bvh, then the texture-slot numbering, then validate_animated_instances.
// scene_materials.h prepare_scene() is that sequence.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/rspt.h"
#include "dev_texture.h"   // RSPT_TEX_MAX_DEPTH; material_assembly.h's rspt_mat::Error

namespace rspt {
namespace scene {

using rspt_mat::Error;

// what the rest of rspt_scene_create reads from validation
struct SceneFacts {
    bool instanced = false;
    uint64_t n_top_prims = 0, n_top_nodes = 0;   // the top-level aggregate's ranges (all of the scene without instances)
    bool has_null = false;                       // some primitive has no material
    bool any_alpha = false;                      // some mesh carries an alpha / shadow-alpha mask
    bool has_maplights = false, has_projection = false, has_goniometric = false;
    bool disk_light = false, cylinder_light = false;
};

inline Error refuse(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return Error{code, buf};
}

// ---- what spheres, disks and cylinders share: two 4x4 matrices, two medium indices, a sweep angle ----
template <class Shape>
bool finite_transforms(const Shape& s) {
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(s.object_to_world[k]) || !std::isfinite(s.world_to_object[k])) return false;
    return true;
}
template <class Shape>
bool media_in_range(const rspt_scene_desc* d, const Shape& s) { return s.medium_inside <= d->n_media && s.medium_outside <= d->n_media; }
inline bool phi_max_in_range(float phi_max) { return phi_max > 0.0f && phi_max <= 2.0f * RSPT_PI; }

inline Error check_arguments(const rspt_scene_desc* d) {
    if (!d) return refuse(RSPT_E_INVALID, "null argument");
    if (d->n_prims > 0x7fffffffull || d->n_nodes > 0x7fffffffull) return refuse(RSPT_E_UNSUPPORTED, "more than 2^31 primitives / nodes");
    if ((d->n_nodes && !d->nodes) || (d->n_prims && (!d->prims || !d->meshes || !d->P)) || (d->n_materials && !d->materials) ||
        (d->n_lights && !d->lights))
        return refuse(RSPT_E_INVALID, "null array with non-zero count");
    if ((d->n_nodes == 0) != (d->n_prims == 0)) return refuse(RSPT_E_INVALID, "nodes and prims must both be empty or both non-empty");
    return Error{};
}

inline Error check_instances(const rspt_scene_desc* d, const SceneFacts& f) {
    if (d->n_spheres && f.instanced) return refuse(RSPT_E_UNSUPPORTED, "spheres together with object instances");   // (ABI 23: a follow-up)
    if (d->n_disks && f.instanced) return refuse(RSPT_E_UNSUPPORTED, "disks together with object instances");
    if (d->n_cylinders && f.instanced) return refuse(RSPT_E_UNSUPPORTED, "cylinders together with object instances");
    if (!f.instanced) return Error{};
    // objects + instances behind the top-level aggregate
    if (!d->instances || !d->objects || d->n_objects == 0) return refuse(RSPT_E_INVALID, "instances without objects");
    if (f.n_top_prims > d->n_prims || f.n_top_nodes > d->n_nodes || f.n_top_nodes == 0) return refuse(RSPT_E_INVALID, "bad top-level aggregate range");
    if (d->instancing_mode != RSPT_INSTANCING_REFERENCE && d->instancing_mode != RSPT_INSTANCING_FIXED) return refuse(RSPT_E_INVALID, "bad instancing_mode");
    for (uint32_t i = 0; i < d->n_objects; i++) {
        const rspt_object& o = d->objects[i];
        if (o.n_prims == 0 || o.first_prim < f.n_top_prims || o.first_prim + o.n_prims > d->n_prims) return refuse(RSPT_E_INVALID, "object %u: primitive range", i);
        if (o.n_nodes == 0 ? o.n_prims != 1 : (o.first_node < f.n_top_nodes || o.first_node + o.n_nodes > d->n_nodes)) return refuse(RSPT_E_INVALID, "object %u: node range", i);
    }
    for (uint32_t i = 0; i < d->n_instances; i++) {
        const rspt_instance& in = d->instances[i];
        if (in.object >= d->n_objects) return refuse(RSPT_E_INVALID, "instance %u: object index out of range", i);
        for (int k = 0; k < 2; k++) {   // (rows 3 other than (0 0 0 1) are served: InstDev::m3 / mi3; a weight of 0 is where the reference asserts, transform.rs:747)
            const float* m = k ? in.from_world : in.to_world;
            if (!std::isfinite(m[12]) || !std::isfinite(m[13]) || !std::isfinite(m[14]) || !std::isfinite(m[15])) return refuse(RSPT_E_INVALID, "instance %u: non-finite transform", i);
            for (int j = 0; j < 12; j++) if (!(fabsf(m[j]) < RSPT_INF)) return refuse(RSPT_E_INVALID, "instance %u: non-finite transform", i);
        }
    }
    return Error{};
}

// ABI 23: spheres (dev_sphere.h); ABI 27: disks and cylinders (dev_quadric.h)
inline Error check_shapes(const rspt_scene_desc* d) {
    if (d->n_spheres && !d->spheres) return refuse(RSPT_E_INVALID, "null spheres with n_spheres > 0");
    for (uint32_t i = 0; i < d->n_spheres; i++) {
        const rspt_sphere& sp = d->spheres[i];
        if (!finite_transforms(sp)) return refuse(RSPT_E_INVALID, "sphere %u: non-finite transform", i);
        if (!(sp.radius > 0.0f) || !std::isfinite(sp.radius) || !std::isfinite(sp.z_min) || !std::isfinite(sp.z_max) || !std::isfinite(sp.phi_max) ||
            !std::isfinite(sp.theta_min) || !std::isfinite(sp.theta_max))
            return refuse(RSPT_E_INVALID, "sphere %u: radius must be positive and finite, z / theta / phi finite", i);
        if (!media_in_range(d, sp)) return refuse(RSPT_E_INVALID, "sphere %u: medium index out of range", i);
    }
    if (d->n_disks && !d->disks) return refuse(RSPT_E_INVALID, "null disks with n_disks > 0");
    if (d->n_cylinders && !d->cylinders) return refuse(RSPT_E_INVALID, "null cylinders with n_cylinders > 0");
    if ((uint64_t)d->n_spheres + d->n_disks + d->n_cylinders > 0x7fffffffull) return refuse(RSPT_E_UNSUPPORTED, "more than 2^31 spheres, disks and cylinders");
    for (uint32_t i = 0; i < d->n_disks; i++) {
        const rspt_disk& k = d->disks[i];
        if (!finite_transforms(k)) return refuse(RSPT_E_INVALID, "disk %u: non-finite transform", i);
        if (!std::isfinite(k.height) || !std::isfinite(k.radius) || !std::isfinite(k.inner_radius) || !std::isfinite(k.phi_max)) return refuse(RSPT_E_INVALID, "disk %u: non-finite parameter", i);
        if (!(k.radius > 0.0f)) return refuse(RSPT_E_INVALID, "disk %u: radius must be positive", i);
        if (k.radius == k.inner_radius) return refuse(RSPT_E_INVALID, "disk %u: radius equals inner_radius (v divides by their difference)", i);
        if (!phi_max_in_range(k.phi_max)) return refuse(RSPT_E_INVALID, "disk %u: phi_max outside (0, 2 pi]", i);
        if (!media_in_range(d, k)) return refuse(RSPT_E_INVALID, "disk %u: medium index out of range", i);
    }
    for (uint32_t i = 0; i < d->n_cylinders; i++) {
        const rspt_cylinder& k = d->cylinders[i];
        if (!finite_transforms(k)) return refuse(RSPT_E_INVALID, "cylinder %u: non-finite transform", i);
        if (!std::isfinite(k.radius) || !std::isfinite(k.z_min) || !std::isfinite(k.z_max) || !std::isfinite(k.phi_max)) return refuse(RSPT_E_INVALID, "cylinder %u: non-finite parameter", i);
        if (!(k.radius > 0.0f)) return refuse(RSPT_E_INVALID, "cylinder %u: radius must be positive", i);
        if (k.z_min == k.z_max) return refuse(RSPT_E_INVALID, "cylinder %u: z_min equals z_max (v divides by their difference)", i);
        if (!phi_max_in_range(k.phi_max)) return refuse(RSPT_E_INVALID, "cylinder %u: phi_max outside (0, 2 pi]", i);
        if (!media_in_range(d, k)) return refuse(RSPT_E_INVALID, "cylinder %u: medium index out of range", i);
    }
    return Error{};
}

// a sphere, disk or cylinder primitive: v[0] names its record; an emissive one's light is a DiffuseAreaLight on this very primitive (the pairing
// api.rs makes, and rspt_light.prim states).  (The sphere's material refusal is worded without the shape's name.)
inline Error check_analytic_prim(const rspt_scene_desc* d, uint64_t i, const rspt_prim& p, const char* kn, uint32_t n_shapes) {
    const unsigned long long ii = (unsigned long long)i;
    if (p.v[0] >= n_shapes) return refuse(RSPT_E_INVALID, "prim %llu: %s index out of range", ii, kn);
    if (p.material != 0xffffffffu && p.material >= d->n_materials)
        return p.mesh == RSPT_MESH_SPHERE ? refuse(RSPT_E_INVALID, "prim %llu: material index out of range", ii) : refuse(RSPT_E_INVALID, "prim %llu: %s's material index out of range", ii, kn);
    if (p.area_light < -1 || p.area_light >= (int64_t)d->n_lights) return refuse(RSPT_E_INVALID, "prim %llu: %s's light index out of range", ii, kn);
    if (p.area_light >= 0 && (d->lights[p.area_light].kind != RSPT_LIGHT_DIFFUSE_AREA || d->lights[p.area_light].prim != i))
        return refuse(RSPT_E_INVALID, "prim %llu: %s's area light %d is not a DIFFUSE_AREA light on this primitive", ii, kn, p.area_light);
    return Error{};
}

inline Error check_prims(const rspt_scene_desc* d, SceneFacts* f) {
    for (uint64_t i = 0; i < d->n_prims; i++) {
        const rspt_prim& p = d->prims[i];
        const unsigned long long ii = (unsigned long long)i;
        if (p.mesh == RSPT_MESH_SPHERE || p.mesh == RSPT_MESH_DISK || p.mesh == RSPT_MESH_CYLINDER) {
            const bool sp = p.mesh == RSPT_MESH_SPHERE, dk = p.mesh == RSPT_MESH_DISK;
            if (Error e = check_analytic_prim(d, i, p, sp ? "sphere" : (dk ? "disk" : "cylinder"), sp ? d->n_spheres : (dk ? d->n_disks : d->n_cylinders))) return e;
            if (!sp && p.area_light >= 0) (dk ? f->disk_light : f->cylinder_light) = true;
            f->has_null |= p.material == 0xffffffffu;
            continue;
        }
        if (p.mesh == RSPT_MESH_INSTANCE) {
            if (!f->instanced || i >= f->n_top_prims || p.v[0] >= d->n_instances) return refuse(RSPT_E_INVALID, "prim %llu: bad instance reference", ii);
            continue;
        }
        if (i >= f->n_top_prims && p.area_light != -1) return refuse(RSPT_E_UNSUPPORTED, "prim %llu: area lights are not supported with object instancing (api.rs:2899)", ii);
        if (p.v[0] >= d->n_vertices || p.v[1] >= d->n_vertices || p.v[2] >= d->n_vertices) return refuse(RSPT_E_INVALID, "prim %llu: vertex index out of range", ii);
        if (p.mesh >= d->n_meshes) return refuse(RSPT_E_INVALID, "prim %llu: mesh index out of range", ii);
        if (p.material != 0xffffffffu && p.material >= d->n_materials) return refuse(RSPT_E_INVALID, "prim %llu: material index out of range", ii);
        if (p.area_light >= (int64_t)d->n_lights) return refuse(RSPT_E_INVALID, "prim %llu: light index out of range", ii);
        f->has_null |= p.material == 0xffffffffu;
    }
    return Error{};
}

inline Error check_meshes(const rspt_scene_desc* d, SceneFacts* f) {
    for (uint32_t i = 0; i < d->n_meshes; i++) {
        const rspt_mesh& m = d->meshes[i];
        if (m.alpha_tex > d->n_textures || m.shadow_alpha_tex > d->n_textures) return refuse(RSPT_E_INVALID, "mesh %u: alpha texture index out of range", i);
        f->any_alpha |= m.alpha_tex != 0 || m.shadow_alpha_tex != 0;
        if (m.medium_inside > d->n_media || m.medium_outside > d->n_media) return refuse(RSPT_E_INVALID, "mesh %u: medium index out of range", i);
    }
    return Error{};
}

inline Error check_media(const rspt_scene_desc* d) {
    if (d->n_media && !d->media) return refuse(RSPT_E_INVALID, "null media");
    for (uint32_t i = 0; i < d->n_media; i++) {
        const rspt_medium& m = d->media[i];
        if (m.kind != RSPT_MEDIUM_HOMOGENEOUS && m.kind != RSPT_MEDIUM_GRID) return refuse(RSPT_E_UNSUPPORTED, "medium %u: kind %u (homogeneous and grid-density media)", i, m.kind);
        if (m.kind == RSPT_MEDIUM_GRID) {
            if (m.nx < 1 || m.ny < 1 || m.nz < 1 || (uint64_t)m.nx * m.ny * m.nz > (1ull << 31) || !m.density) return refuse(RSPT_E_INVALID, "medium %u: bad density grid", i);
            const float* w = m.world_to_medium;
            if (w[12] != 0.0f || w[13] != 0.0f || w[14] != 0.0f || w[15] != 1.0f) return refuse(RSPT_E_UNSUPPORTED, "medium %u: projective world_to_medium", i);
        }
        for (int c = 0; c < 3; c++)
            if (!(m.sigma_a[c] >= 0.0f) || !(m.sigma_s[c] >= 0.0f) || !std::isfinite(m.sigma_a[c]) || !std::isfinite(m.sigma_s[c])) return refuse(RSPT_E_INVALID, "medium %u: bad sigma_a / sigma_s", i);
        if (!(m.g > -1.0f && m.g < 1.0f)) return refuse(RSPT_E_INVALID, "medium %u: g outside (-1, 1)", i);
    }
    return Error{};
}

inline Error check_emissive_alpha(const rspt_scene_desc* d, const SceneFacts& f) {
    if (!f.any_alpha) return Error{};
    for (uint64_t i = 0; i < d->n_prims; i++) {
        const rspt_prim& p = d->prims[i];
        if (p.mesh < d->n_meshes && p.area_light >= 0 && (d->meshes[p.mesh].alpha_tex || d->meshes[p.mesh].shadow_alpha_tex))
            return refuse(RSPT_E_UNSUPPORTED, "prim %llu: an emissive mesh with an alpha mask", (unsigned long long)i);
    }
    return Error{};
}

inline Error check_lights(const rspt_scene_desc* d, SceneFacts* f) {
    for (uint32_t i = 0; i < d->n_lights; i++) {
        const rspt_light& l = d->lights[i];
        if (l.kind < RSPT_LIGHT_DIFFUSE_AREA || l.kind > RSPT_LIGHT_GONIOMETRIC) return refuse(RSPT_E_UNSUPPORTED, "light %u: unsupported kind %u", i, l.kind);
        if (l.kind == RSPT_LIGHT_DIFFUSE_AREA) {
            if (l.prim >= f->n_top_prims || d->prims[l.prim].mesh == RSPT_MESH_INSTANCE) return refuse(RSPT_E_INVALID, "light %u: prim out of range", i);   // (a sphere primitive may be named, ABI 23)
            const rspt_prim& p = d->prims[l.prim];
            if (p.mesh == RSPT_MESH_SPHERE && p.area_light != (int32_t)i) return refuse(RSPT_E_INVALID, "light %u: its sphere primitive names another light", i);
            if ((p.mesh == RSPT_MESH_DISK || p.mesh == RSPT_MESH_CYLINDER) && p.area_light != (int32_t)i)
                return refuse(RSPT_E_INVALID, "light %u: its %s primitive names another light", i, p.mesh == RSPT_MESH_DISK ? "disk" : "cylinder");
        }
        if (l.kind == RSPT_LIGHT_INFINITE && l.prim >= d->n_envmaps) return refuse(RSPT_E_INVALID, "light %u: envmap index out of range", i);
        if (l.kind == RSPT_LIGHT_PROJECTION || l.kind == RSPT_LIGHT_GONIOMETRIC) {   // ABI 24
            const char* kn = l.kind == RSPT_LIGHT_PROJECTION ? "projection" : "goniometric";
            const int n_par = l.kind == RSPT_LIGHT_PROJECTION ? 22 : 12;
            for (int k = 0; k < 3; k++) if (!std::isfinite(l.L[k])) return refuse(RSPT_E_INVALID, "light %u (%s): non-finite intensity", i, kn);
            for (int k = 0; k < n_par; k++) if (!std::isfinite(l.p[k])) return refuse(RSPT_E_INVALID, "light %u (%s): non-finite parameter p[%d]", i, kn, k);
            if (l.prim != 0xffffffffu && l.prim >= d->n_envmaps) return refuse(RSPT_E_INVALID, "light %u (%s): map index out of range", i, kn);
            if (l.kind == RSPT_LIGHT_PROJECTION && (l.p[12] > l.p[14] || l.p[13] > l.p[15])) return refuse(RSPT_E_INVALID, "light %u (projection): screen_bounds min above max", i);
            f->has_maplights = true;
            (l.kind == RSPT_LIGHT_PROJECTION ? f->has_projection : f->has_goniometric) = true;
        }
    }
    return Error{};
}

// an image's or an envmap's pyramid: power-of-two sides up to 32768, one level per halving of the longer side
inline Error check_pyramid(const char* what, const char* sides_note, uint32_t i, uint32_t width, uint32_t height, uint32_t n_levels) {
    auto pow2 = [](uint32_t v) { return v && !(v & (v - 1)); };
    if (!pow2(width) || !pow2(height) || width > 32768 || height > 32768) return refuse(RSPT_E_INVALID, "%s %u: sides must be powers of two <= 32768%s", what, i, sides_note);
    uint32_t nl = 1;
    for (uint32_t m = std::max(width, height); m > 1; m >>= 1) nl++;
    if (n_levels != nl || nl > 16) return refuse(RSPT_E_INVALID, "%s %u: n_levels %u, expected %u", what, i, n_levels, nl);
    return Error{};
}

// textures: constant / imagemap / scale; each material may bind at most RSPT_TEX_SLOTS distinct ones
inline Error check_images(const rspt_scene_desc* d) {
    if ((d->n_textures && !d->textures) || (d->n_images && !d->images)) return refuse(RSPT_E_INVALID, "null texture / image array");
    for (uint32_t i = 0; i < d->n_images; i++) {
        const rspt_image& im = d->images[i];
        if (Error e = check_pyramid("image", " (MipMap::new resamples first)", i, im.width, im.height, im.n_levels)) return e;
        if (!im.texels || (im.channels != 1 && im.channels != 3)) return refuse(RSPT_E_INVALID, "image %u: null texels or channels not 1 / 3", i);
    }
    return Error{};
}

// nodes on the longest path below texture i; 1000 and more: a child index out of range or a cycle.  depth[]: 0 = not computed, -1 = on the current path
inline int texture_depth(const rspt_scene_desc* d, std::vector<int>& depth, uint32_t i) {
    if (depth[i] > 0) return depth[i];
    if (depth[i] < 0) return 1000;
    depth[i] = -1;
    const rspt_texture& t = d->textures[i];
    int dmax = 0;
    const uint32_t kids[3] = {t.tex1, t.tex2, t.tex3};
    const int n_kids = t.kind == RSPT_TEX_MIX ? 3 : ((t.kind == RSPT_TEX_SCALE || t.kind == RSPT_TEX_CHECKERBOARD || t.kind == RSPT_TEX_DOTS) ? 2 : 0);
    for (int k = 0; k < n_kids; k++) dmax = std::max(dmax, kids[k] < d->n_textures ? texture_depth(d, depth, kids[k]) : 1000);
    return depth[i] = 1 + dmax;
}

// texture graph: kinds, mappings, child indices, depth (dev_texture.h evaluates at most RSPT_TEX_MAX_DEPTH levels)
inline Error check_texture_graph(const rspt_scene_desc* d) {
    std::vector<int> depth(d->n_textures, 0);
    for (uint32_t i = 0; i < d->n_textures; i++) {
        const rspt_texture& t = d->textures[i];
        if (t.kind < RSPT_TEX_CONSTANT || t.kind > RSPT_TEX_WRINKLED) return refuse(RSPT_E_UNSUPPORTED, "texture %u: unsupported kind %u", i, t.kind);
        const bool map2d = t.kind == RSPT_TEX_IMAGE || t.kind == RSPT_TEX_CHECKERBOARD || t.kind == RSPT_TEX_DOTS;
        const bool map3d = t.kind == RSPT_TEX_FBM || t.kind == RSPT_TEX_MARBLE || t.kind == RSPT_TEX_WINDY || t.kind == RSPT_TEX_WRINKLED;
        if (map2d && (t.mapping < RSPT_MAP_UV || t.mapping > RSPT_MAP_CYLINDRICAL)) return refuse(RSPT_E_UNSUPPORTED, "texture %u: 2-D mapping %u", i, t.mapping);
        if (map3d && t.mapping != RSPT_MAP_IDENTITY3D) return refuse(RSPT_E_UNSUPPORTED, "texture %u: 3-D textures take the identity mapping", i);
        if (map3d && (t.octaves < 0 || t.octaves > 64)) return refuse(RSPT_E_INVALID, "texture %u: octaves out of range", i);
        if (t.kind == RSPT_TEX_IMAGE) {
            if (t.image >= d->n_images) return refuse(RSPT_E_INVALID, "texture %u: image index out of range", i);
            if (t.wrap > RSPT_WRAP_CLAMP) return refuse(RSPT_E_INVALID, "texture %u: bad wrap mode", i);
        }
        const int dep = texture_depth(d, depth, i);
        if (dep >= 1000) return refuse(RSPT_E_INVALID, "texture %u: child index out of range or cyclic graph", i);
        if (dep > RSPT_TEX_MAX_DEPTH) return refuse(RSPT_E_UNSUPPORTED, "texture %u: graph deeper than %d levels", i, RSPT_TEX_MAX_DEPTH);
    }
    return Error{};
}

// Everything up to the material assembly.
inline Error validate_scene(const rspt_scene_desc* d, SceneFacts* out) {
    *out = SceneFacts{};
    if (Error e = check_arguments(d)) return e;
    SceneFacts& f = *out;
    f.instanced = d->n_instances > 0;
    f.n_top_prims = f.instanced ? d->n_top_prims : d->n_prims;
    f.n_top_nodes = f.instanced ? d->n_top_nodes : d->n_nodes;
    Error e;
    if ((e = check_instances(d, f)) || (e = check_shapes(d)) || (e = check_prims(d, &f)) || (e = check_meshes(d, &f)) || (e = check_media(d)) ||
        (e = check_emissive_alpha(d, f)) || (e = check_lights(d, &f)) || (e = check_images(d)) || (e = check_texture_graph(d)))
        return e;
    return Error{};
}

inline Error check_envmaps(const rspt_scene_desc* d) {
    if (d->n_envmaps && !d->envmaps) return refuse(RSPT_E_INVALID, "null envmaps");
    for (uint32_t i = 0; i < d->n_envmaps; i++) {
        const rspt_envmap& e = d->envmaps[i];
        if (Error er = check_pyramid("envmap", "", i, e.width, e.height, e.n_levels)) return er;
        // ABI 24: a map that only projection / goniometric lights name carries no distribution (they never sample it); an infinite light needs its own
        bool sampled = false, named = false;
        for (uint32_t l = 0; l < d->n_lights; l++) {
            if (d->lights[l].kind == RSPT_LIGHT_INFINITE && d->lights[l].prim == i) sampled = true;
            if ((d->lights[l].kind == RSPT_LIGHT_PROJECTION || d->lights[l].kind == RSPT_LIGHT_GONIOMETRIC) && d->lights[l].prim == i) named = true;
        }
        const bool no_dist = !e.dist_func && e.dist_nu == 0 && e.dist_nv == 0;
        if (!e.texels || !((named && !sampled && no_dist) || (e.dist_func && e.dist_nu != 0 && e.dist_nv != 0))) return refuse(RSPT_E_INVALID, "envmap %u: null data", i);
    }
    return Error{};
}

// levels of the tree at `root` whose nodes lie in [node_lo, node_hi) and whose leaves in [prim_lo, prim_hi); -1 (malformed) or -2 (too deep) with *err set
inline int bvh_tree_depth(const rspt_scene_desc* d, uint64_t root, uint64_t node_lo, uint64_t node_hi, uint64_t prim_lo, uint64_t prim_hi, std::string* err) {
    std::vector<std::pair<uint32_t, uint32_t>> stack;  // node, depth
    stack.push_back({(uint32_t)root, 1u});
    uint64_t visited = 0;
    uint32_t deepest = 0;
    while (!stack.empty()) {
        auto [ni, depth] = stack.back();
        stack.pop_back();
        if (++visited > node_hi - node_lo) { *err = "BVH is not a tree"; return -1; }
        deepest = std::max(deepest, depth);
        if (depth > 64) { *err = "BVH deeper than the 64-entry traversal stack"; return -2; }
        const rspt_bvh_node& n = d->nodes[ni];
        if (n.n_prims > 0) {
            if (n.offset < 0 || (uint64_t)n.offset < prim_lo || (uint64_t)n.offset + n.n_prims > prim_hi) { *err = "node " + std::to_string(ni) + ": leaf range out of bounds"; return -1; }
        } else {
            if (n.axis > 2 || n.offset <= (int64_t)ni || (uint64_t)n.offset >= node_hi || (uint64_t)ni + 1 >= node_hi) { *err = "node " + std::to_string(ni) + ": bad children"; return -1; }
            stack.push_back({(uint32_t)n.offset, depth + 1});
            stack.push_back({ni + 1, depth + 1});
        }
    }
    return (int)deepest;
}

// BVH: child / leaf ranges in bounds, depth <= 64 (the reference's fixed traversal stack, bvh.rs:420); with instances the
// object's traversal continues on the stack of the top-level one (kernels.h traverse), so the two depths add up
inline Error check_bvh(const rspt_scene_desc* d, const SceneFacts& f) {
    std::string err;
    int top_depth = 0, obj_depth = 0;
    if (d->n_nodes) {
        top_depth = bvh_tree_depth(d, 0, 0, f.n_top_nodes, 0, f.n_top_prims, &err);
        if (top_depth < 0) return refuse(top_depth == -2 ? RSPT_E_UNSUPPORTED : RSPT_E_INVALID, "%s", err.c_str());
    }
    for (uint32_t i = 0; f.instanced && i < d->n_objects; i++) {
        const rspt_object& o = d->objects[i];
        if (o.n_nodes == 0) continue;
        const int dep = bvh_tree_depth(d, o.first_node, o.first_node, o.first_node + o.n_nodes, o.first_prim, o.first_prim + o.n_prims, &err);
        if (dep < 0) return refuse(dep == -2 ? RSPT_E_UNSUPPORTED : RSPT_E_INVALID, "object %u: %s", i, err.c_str());
        obj_depth = std::max(obj_depth, dep);
    }
    if (top_depth + obj_depth > 64) return refuse(RSPT_E_UNSUPPORTED, "top-level BVH (%d levels) + object BVH (%d levels) deeper than the 64-entry traversal stack", top_depth, obj_depth);
    return Error{};
}

// What follows the material assembly.
inline Error validate_envmaps_and_bvh(const rspt_scene_desc* d, const SceneFacts& f) {
    if (Error e = check_envmaps(d)) return e;
    return check_bvh(d, f);
}

// A moving instance (ABI 20): its two key times and its end key.  The last validation step, behind the texture-slot numbering.
inline Error validate_animated_instances(const rspt_scene_desc* d) {
    for (uint32_t i = 0; i < d->n_instances; i++) {
        const rspt_instance& in = d->instances[i];
        if (!in.animated) continue;
        if (!std::isfinite(in.time[0]) || !std::isfinite(in.time[1]) || !(in.time[1] > in.time[0]))
            return refuse(RSPT_E_INVALID, "instance %u: animated with time[1] <= time[0] or a non-finite key time", i);
        for (int k = 0; k < 16; k++)
            if (!std::isfinite(in.to_world_end[k]) || !std::isfinite(in.from_world_end[k]))
                return refuse(RSPT_E_INVALID, "instance %u: non-finite end key matrix", i);
        // transform_point divides by the homogeneous weight and the reference asserts it is not zero (transform.rs:505): an end key whose
        // rows 3 are all zero can only produce such weights
        if (in.to_world_end[12] == 0.0f && in.to_world_end[13] == 0.0f && in.to_world_end[14] == 0.0f && in.to_world_end[15] == 0.0f)
            return refuse(RSPT_E_INVALID, "instance %u: end key with a zero homogeneous row", i);
        if (in.from_world_end[12] == 0.0f && in.from_world_end[13] == 0.0f && in.from_world_end[14] == 0.0f && in.from_world_end[15] == 0.0f)
            return refuse(RSPT_E_INVALID, "instance %u: end key inverse with a zero homogeneous row", i);
    }
    return Error{};
}

}  // namespace scene
}  // namespace rspt
