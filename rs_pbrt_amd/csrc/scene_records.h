// rs_pbrt_amd — the records rspt_scene_create uploads, built in plain host arithmetic from an rspt_scene_desc that scene_validate.h has
// passed: the four-box records of trace_w4.h and their 8-bit form (trace_w4q.h), leaf boxes, the pair records of trace_wide.h, the in-line
// alpha masks, the instance records, image pyramids, envmap distributions, the sphere / disk / cylinder slots.  No HIP runtime call: the
// types come from the kernels' headers, the work is the host's, and tests/scene_host_main.hip checks the records' invariants without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "camera_anim.h"
#include "dev_quadric.h"
#include "dev_texture.h"
#include "scene_validate.h"
#include "trace_w4.h"
#include "trace_w4q.h"
#include "trace_wide.h"

namespace rspt {
namespace scene {

// ---- four-box records (trace_w4.h): grandchildren of every interior node at even depth; with object instances every object's
// aggregate gets its own records behind the top-level ones, and every instance primitive the reference to the rest of its leaf ----
struct W4Records {
    std::vector<Wide4Node> recs;
    std::vector<uint2> big_leaves;        // (offset, count) of the leaves a ref's fields cannot hold
    uint32_t w4_root = 0;                 // record 0, or a leaf reference when the root is a leaf
    uint32_t w4_top = 0;                  // the breadth-first prefix numbered first
    std::vector<uint32_t> obj_root;       // per object: its aggregate's first record, or a leaf reference
    std::vector<uint32_t> inst_cont;      // per instance: the primitives behind it in its top-level leaf (RSPT_NONE: it is the last)
    bool w4_ok = false;                   // false: too large for the ref fields (or no nodes at all)
};

inline uint32_t range_ref(std::vector<uint2>& big, uint32_t off, uint32_t cnt) {
    if (cnt <= 15u && off <= RSPT_W4_OFFSET_MASK) return RSPT_REF_LEAF | ((cnt - 1u) << RSPT_W4_COUNT_SHIFT) | off;
    big.push_back(make_uint2(off, cnt));
    return RSPT_REF_LEAF | (15u << RSPT_W4_COUNT_SHIFT) | (uint32_t)(big.size() - 1);
}

inline uint32_t leaf_ref(const rspt_scene_desc* d, const SceneFacts& f, W4Records& out, uint32_t ni) {
    const rspt_bvh_node& n = d->nodes[ni];
    if (f.instanced && ni < f.n_top_nodes)  // an instance in this leaf: the primitives behind it are reached again through its continuation reference
        for (uint32_t i = 0; i + 1u < n.n_prims; i++) {
            const rspt_prim& p = d->prims[(uint32_t)n.offset + i];
            if (p.mesh == RSPT_MESH_INSTANCE) out.inst_cont[p.v[0]] = range_ref(out.big_leaves, (uint32_t)n.offset + i + 1u, n.n_prims - i - 1u);
        }
    return range_ref(out.big_leaves, (uint32_t)n.offset, n.n_prims);
}

// the records of the tree rooted at LinearBVHNode `root` (an interior node), depth first, with record-local indices
inline void build_tree(const rspt_scene_desc* d, const SceneFacts& f, W4Records& out, uint32_t root, std::vector<Wide4Node>& recs, std::vector<uint32_t>& rec_axes) {
    const float qnan = std::numeric_limits<float>::quiet_NaN();
    std::vector<std::pair<uint32_t, uint32_t>> todo;  // (LinearBVHNode index, record index)
    recs.clear(); rec_axes.assign(1, 0u);
    recs.emplace_back();
    todo.emplace_back(root, 0u);
    while (!todo.empty()) {
        const auto [ai, ri] = todo.back();
        todo.pop_back();
        const rspt_bvh_node& a = d->nodes[ai];
        uint32_t slot_node[4] = {RSPT_NONE, RSPT_NONE, RSPT_NONE, RSPT_NONE};
        uint32_t axes = a.axis;
        const uint32_t child[2] = {ai + 1u, (uint32_t)a.offset};
        for (int gi = 0; gi < 2; gi++) {
            const rspt_bvh_node& c = d->nodes[child[gi]];
            if (c.n_prims != 0) {
                slot_node[2 * gi] = child[gi];
            } else {
                axes |= (uint32_t)c.axis << (2 + 2 * gi);
                slot_node[2 * gi] = child[gi] + 1u;
                slot_node[2 * gi + 1] = (uint32_t)c.offset;
            }
        }
        Wide4Node w{};
        float lo[4][3], hi[4][3];
        uint32_t pending[4], n_pending = 0;
        for (int k = 0; k < 4; k++) {
            if (slot_node[k] == RSPT_NONE) {
                for (int c = 0; c < 3; c++) lo[k][c] = hi[k][c] = qnan;
                w.ref[k] = RSPT_NONE;
                continue;
            }
            const rspt_bvh_node& x = d->nodes[slot_node[k]];
            for (int c = 0; c < 3; c++) { lo[k][c] = x.bmin[c]; hi[k][c] = x.bmax[c]; }
            if (x.n_prims != 0) w.ref[k] = leaf_ref(d, f, out, slot_node[k]);
            else pending[n_pending++] = (uint32_t)k;
        }
        // children records are numbered so that the first slot's subtree follows its parent (pushed last)
        for (uint32_t j = 0; j < n_pending; j++) { w.ref[pending[j]] = (uint32_t)recs.size(); recs.emplace_back(); rec_axes.push_back(0u); }
        for (uint32_t j = n_pending; j-- > 0;) todo.emplace_back(slot_node[pending[j]], w.ref[pending[j]]);
        for (int c = 0; c < 3; c++) {
            w.b[c] = make_float4(lo[0][c], lo[1][c], hi[0][c], hi[1][c]);
            w.b[3 + c] = make_float4(lo[2][c], lo[3][c], hi[2][c], hi[3][c]);
        }
        rec_axes[ri] = axes;
        recs[ri] = w;
    }
}

// final form of a record: child indices through `new_of` (+ base), the three axes in bits 25..26 of the first three refs (an
// empty slot has a NaN box, its ref is never read as a ref)
inline Wide4Node finish_rec(Wide4Node w, uint32_t axes, const std::vector<uint32_t>* new_of, uint32_t base) {
    for (int k = 0; k < 4; k++)
        if (w.ref[k] != RSPT_NONE && !(w.ref[k] & RSPT_REF_LEAF)) w.ref[k] = (new_of ? (*new_of)[w.ref[k]] : w.ref[k]) + base;
    for (int k = 0; k < 3; k++) w.ref[k] = (w.ref[k] & ~RSPT_W4_AXIS_MASK) | (((axes >> (2 * k)) & 3u) << RSPT_W4_AXIS_SHIFT);
    return w;
}

inline W4Records build_w4(const rspt_scene_desc* d, const SceneFacts& f) {
    W4Records out;
    out.obj_root.assign(d->n_objects, RSPT_NONE);
    out.inst_cont.assign(d->n_instances, RSPT_NONE);
    if (d->n_nodes == 0) return out;
    std::vector<Wide4Node>& recs = out.recs;
    std::vector<Wide4Node> local;
    std::vector<uint32_t> axes;
    if (d->nodes[0].n_prims != 0) {
        out.w4_root = leaf_ref(d, f, out, 0);
    } else {
        build_tree(d, f, out, 0u, local, axes);
        // Renumber: a breadth-first prefix of RSPT_W4_TOP_MAX records goes first (k_trace_w4 keeps its first TOPCAP in LDS: any prefix of a
        // breadth-first order is one), the others keep their depth-first order.
        std::vector<uint32_t> new_of(local.size(), RSPT_NONE), order(1, 0u);
        for (size_t h = 0; h < order.size() && order.size() < RSPT_W4_TOP_MAX; h++)
            for (int k = 0; k < 4; k++) {
                const uint32_t r = local[order[h]].ref[k];
                if (r != RSPT_NONE && !(r & RSPT_REF_LEAF) && order.size() < RSPT_W4_TOP_MAX) order.push_back(r);
            }
        for (size_t i = 0; i < order.size(); i++) new_of[order[i]] = (uint32_t)i;
        uint32_t next_index = (uint32_t)order.size();
        for (size_t i = 0; i < local.size(); i++)
            if (new_of[i] == RSPT_NONE) new_of[i] = next_index++;
        recs.resize(local.size());
        for (size_t i = 0; i < local.size(); i++) recs[new_of[i]] = finish_rec(local[i], axes[i], &new_of, 0u);
        out.w4_top = (uint32_t)order.size();
        out.w4_root = 0u;
    }
    for (uint32_t o = 0; f.instanced && o < d->n_objects; o++) {
        const rspt_object& ob = d->objects[o];
        if (ob.n_nodes == 0) out.obj_root[o] = range_ref(out.big_leaves, (uint32_t)ob.first_prim, 1u);                  // a lone primitive: no box, no aggregate
        else if (d->nodes[ob.first_node].n_prims != 0) out.obj_root[o] = leaf_ref(d, f, out, (uint32_t)ob.first_node);  // a one-leaf aggregate
        else {
            build_tree(d, f, out, (uint32_t)ob.first_node, local, axes);
            const uint32_t base = (uint32_t)recs.size();
            for (size_t i = 0; i < local.size(); i++) recs.push_back(finish_rec(local[i], axes[i], nullptr, base));
            out.obj_root[o] = base;
        }
    }
    // record indices and big-leaf indices must leave bits 25..30 free; larger scenes stay on the two-box kernel
    out.w4_ok = recs.size() <= RSPT_W4_OFFSET_MASK && out.big_leaves.size() <= RSPT_W4_OFFSET_MASK;
    return out;
}

// ---- the quantised form of the records (trace_w4q.h): false when some box is not finite or does not fit the grid ----
inline bool quantise_w4(const std::vector<Wide4Node>& recs, std::vector<Quad4Node>* out) {
    std::vector<Quad4Node>& q = *out;
    q.resize(recs.size());
    bool ok = true;
    for (size_t i = 0; i < recs.size() && ok; i++) {
        const Wide4Node& w = recs[i];
        Quad4Node& o = q[i];
        memset(&o, 0, sizeof o);
        memcpy(o.ref, w.ref, sizeof o.ref);
        uint32_t qlo[3] = {0, 0, 0}, qhi[3] = {0, 0, 0}, meta = 0;
        for (int c = 0; c < 3 && ok; c++) {
            const float lo4[4] = {w.b[c].x, w.b[c].y, w.b[3 + c].x, w.b[3 + c].y}, hi4[4] = {w.b[c].z, w.b[c].w, w.b[3 + c].z, w.b[3 + c].w};
            double org = 0.0, top = 0.0;
            bool have = false;
            for (int k = 0; k < 4; k++) {
                if (lo4[k] != lo4[k]) { if (c == 0) meta |= 1u << (24 + k); continue; }   // an empty slot: a NaN box
                org = have ? std::min(org, (double)lo4[k]) : (double)lo4[k];
                top = have ? std::max(top, (double)hi4[k]) : (double)hi4[k];
                have = true;
            }
            if (!have) { o.org[c] = 0.0f; meta |= 100u << (8 * c); continue; }
            if (!std::isfinite(org) || !std::isfinite(top)) { ok = false; break; }
            // cell = 2^(e - 127), the smallest power of two with 255 cells covering the extent (never below 2^-67, never above 2^60)
            int e = 60;
            if (top > org) { int ex = 0; (void)std::frexp((top - org) / 255.0, &ex); e = std::max(60, std::min(187, ex + 127 - 2)); }   // (start two below the answer: the loop then takes <= 3 steps)
            while (e < 187 && std::ceil((top - org) / std::ldexp(1.0, e - 127)) > 255.0) e++;
            if (std::ceil((top - org) / std::ldexp(1.0, e - 127)) > 255.0) { ok = false; break; }
            const double cell = std::ldexp(1.0, e - 127);
            o.org[c] = (float)org;   // (org is one of the f32 planes: exact)
            meta |= (uint32_t)e << (8 * c);
            for (int k = 0; k < 4; k++) {
                if (lo4[k] != lo4[k]) { qlo[c] |= 255u << (8 * k); continue; }   // empty: lower plane above the upper one (and the empty bit)
                const double fl = std::floor(((double)lo4[k] - org) / cell), ce = std::ceil(((double)hi4[k] - org) / cell);
                const uint32_t a = (uint32_t)std::min(255.0, std::max(0.0, fl)), b = (uint32_t)std::min(255.0, std::max(0.0, ce));
                if (org + a * cell > (double)lo4[k] || org + b * cell < (double)hi4[k]) { ok = false; break; }   // outward, in exact arithmetic
                qlo[c] |= a << (8 * k); qhi[c] |= b << (8 * k);
            }
        }
        o.meta = meta; o.qlo[0] = qlo[0]; o.qlo[1] = qlo[1]; o.qlo[2] = qlo[2]; o.qhi_x = qhi[0]; o.qhi_y = qhi[1]; o.qhi_z = qhi[2];
    }
    return ok;
}

// [2 * first primitive of a leaf]: the leaf's LinearBVHNode bounds, in the layout box_hit reads (sc.nodes)
inline std::vector<float4> leaf_boxes(const rspt_scene_desc* d) {
    std::vector<float4> lb(2 * (size_t)d->n_prims, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint64_t ni = 0; ni < d->n_nodes; ni++) {
        const rspt_bvh_node& n = d->nodes[ni];
        if (n.n_prims == 0) continue;
        lb[2 * (size_t)n.offset] = make_float4(n.bmin[0], n.bmin[1], n.bmin[2], n.bmax[0]);
        lb[2 * (size_t)n.offset + 1] = make_float4(n.bmax[1], n.bmax[2], 0.0f, 0.0f);
    }
    return lb;
}

// pair records: both children's boxes next to each other (trace_wide.h), one per interior node
inline std::vector<PairNode> build_pairs(const rspt_scene_desc* d) {
    std::vector<uint32_t> pair_of(d->n_nodes, 0u);
    uint32_t n_pairs = 0;
    for (uint64_t i = 0; i < d->n_nodes; i++)
        if (d->nodes[i].n_prims == 0) pair_of[i] = n_pairs++;
    std::vector<PairNode> pairs(n_pairs);
    for (uint64_t i = 0; i < d->n_nodes; i++) {
        const rspt_bvh_node& n = d->nodes[i];
        if (n.n_prims != 0) continue;
        const uint32_t ci[2] = {(uint32_t)i + 1u, (uint32_t)n.offset};
        const rspt_bvh_node& a = d->nodes[ci[0]];
        const rspt_bvh_node& b = d->nodes[ci[1]];
        PairNode& p = pairs[pair_of[i]];
        p.q0 = make_float4(a.bmin[0], b.bmin[0], a.bmax[0], b.bmax[0]);
        p.q1 = make_float4(a.bmin[1], b.bmin[1], a.bmax[1], b.bmax[1]);
        p.q2 = make_float4(a.bmin[2], b.bmin[2], a.bmax[2], b.bmax[2]);
        p.c0 = a.n_prims ? (ci[0] | RSPT_REF_LEAF) : pair_of[ci[0]];
        p.c1 = b.n_prims ? (ci[1] | RSPT_REF_LEAF) : pair_of[ci[1]];
        p.self = (uint32_t)i;
        p.axis = n.axis;
    }
    return pairs;
}

// ---- alpha masks in the in-line form (dev_scene.h AlphaMask; kernels.h alpha_simple): possible when every mask of the scene is a ConstantTexture or an
// ImageTexture under a UVMapping2D with finite parameters, and meshes with uvs have their per-primitive copies (tri_nuv) ----
struct AlphaMasks {
    std::vector<AlphaEntry> entries;
    std::vector<uint32_t> mesh_mask;   // per mesh: its entry
    bool simple = false;
};
inline bool alpha_mask_of(const rspt_scene_desc* d, const std::vector<uint64_t>& image_base, uint32_t tex_plus_1, AlphaMask* m) {
    memset(m, 0, sizeof *m);
    if (!tex_plus_1) return true;
    const rspt_texture& tx = d->textures[tex_plus_1 - 1u];
    if (tx.kind == RSPT_TEX_CONSTANT) { m->kind = 1u; m->value = tx.value[0]; return true; }
    if (tx.kind != RSPT_TEX_IMAGE || tx.mapping != RSPT_MAP_UV || tx.image >= d->n_images) return false;
    for (int k = 0; k < 4; k++) if (!std::isfinite(tx.map[k])) return false;   // (0 * su must be 0: the lookup's zero differentials)
    const rspt_image& im = d->images[tx.image];
    if (!im.n_levels || im.n_levels > 27u) return false;   // (level = n_levels - 1 + log2(1e-8) must be negative: mipmap.rs:236-239)
    m->kind = 2u; m->su = tx.map[0]; m->sv = tx.map[1]; m->du = tx.map[2]; m->dv = tx.map[3];
    m->width = im.width; m->height = im.height; m->wrap = tx.wrap; m->channels = im.channels; m->base = image_base[tx.image];
    return true;
}
// image_base: per image its first float in the texel pool (empty when the pool was not built); have_tri_nuv: SceneDev::tri_nuv exists
inline AlphaMasks build_alpha_masks(const rspt_scene_desc* d, const std::vector<uint64_t>& image_base, bool have_tri_nuv) {
    AlphaMasks out;
    out.mesh_mask.assign(d->n_meshes, 0u);
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> seen;
    bool simple = image_base.size() == d->n_images;
    for (uint32_t i = 0; i < d->n_meshes && simple; i++) {
        const rspt_mesh& me = d->meshes[i];
        if (!me.alpha_tex && !me.shadow_alpha_tex) continue;
        if (me.has_uv && d->UV && !have_tri_nuv) { simple = false; break; }
        const auto key = std::make_pair(me.alpha_tex, me.shadow_alpha_tex);
        auto it = seen.find(key);
        if (it == seen.end()) {
            AlphaEntry e;
            if (!alpha_mask_of(d, image_base, me.alpha_tex, &e.alpha) || !alpha_mask_of(d, image_base, me.shadow_alpha_tex, &e.shadow) || out.entries.size() >= (1u << (32 - MF_MASK_SHIFT))) { simple = false; break; }
            it = seen.emplace(key, (uint32_t)out.entries.size()).first;
            out.entries.push_back(e);
        }
        out.mesh_mask[i] = it->second;
    }
    out.simple = simple;
    return out;
}

// ---- InstDev records, and InstAnim for the moving ones (ABI 20): AnimatedTransform::new's decomposition of the two keys, as for a moving camera ----
inline void build_instances(const rspt_scene_desc* d, const std::vector<uint32_t>& obj_root, std::vector<InstDev>* ins_out, std::vector<InstAnim>* anims_out) {
    std::vector<InstDev>& ins = *ins_out;
    std::vector<InstAnim>& anims = *anims_out;
    ins.resize(d->n_instances);
    anims.clear();
    for (uint32_t i = 0; i < d->n_instances; i++) {
        const rspt_instance& in = d->instances[i];
        const rspt_object& o = d->objects[in.object];
        InstDev& x = ins[i];
        memset(&x, 0, sizeof x);
        memcpy(x.m, in.to_world, sizeof x.m);
        memcpy(x.mi, in.from_world, sizeof x.mi);
        memcpy(x.m3, in.to_world + 12, sizeof x.m3);
        memcpy(x.mi3, in.from_world + 12, sizeof x.mi3);
        x.root_node = o.n_nodes ? (uint32_t)o.first_node : RSPT_MISS;
        x.first_prim = (uint32_t)o.first_prim;
        x.w4_root = obj_root[in.object];
        bool ident = true;  // Transform::is_identity looks at m only (transform.rs:291-308)
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) ident &= in.to_world[4 * r + c] == (r == c ? 1.0f : 0.0f);
        x.identity = ident ? 1u : 0u;
        x.anim = RSPT_MISS;
        if (!in.animated) continue;
        InstAnim an;
        memset(&an, 0, sizeof an);
        if (camanim::camera_keys(in.to_world, in.time[0], in.to_world_end, in.time[1], &an.keys)) {   // false: equal keys = not actually animated
            memcpy(an.mi_end, in.from_world_end, sizeof an.mi_end);
            bool ie = true;
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) ie &= in.to_world_end[4 * r + c] == (r == c ? 1.0f : 0.0f);
            an.identity_end = ie ? 1u : 0u;
            x.anim = (uint32_t)anims.size();
            anims.push_back(an);
        }
    }
}

// ---- pyramids and envmap distributions ----
// the first texel of every level of a MipMap pyramid; returns the texels of all levels together
inline size_t pyramid_offsets(uint32_t width, uint32_t height, uint32_t n_levels, uint32_t* level_offset) {
    size_t n_tex = 0;
    for (uint32_t l = 0, w = width, h = height; l < n_levels; l++, w = std::max(1u, w / 2), h = std::max(1u, h / 2)) {
        level_offset[l] = (uint32_t)n_tex;
        n_tex += (size_t)w * h;
    }
    return n_tex;
}

// every image's pyramid back to back in one pool; image_base: per image its first float there
inline void build_image_pool(const rspt_scene_desc* d, std::vector<ImageDev>* imgs_out, std::vector<float>* pool_out, std::vector<uint64_t>* image_base) {
    std::vector<ImageDev>& imgs = *imgs_out;
    std::vector<float>& pool = *pool_out;
    imgs.clear(); imgs.resize(d->n_images);
    for (uint32_t i = 0; i < d->n_images; i++) {
        const rspt_image& im = d->images[i];
        ImageDev& o = imgs[i];
        o.width = im.width; o.height = im.height; o.n_levels = im.n_levels; o.channels = im.channels;
        const size_t n_tex = pyramid_offsets(im.width, im.height, im.n_levels, o.level_offset);
        o.texel_base = pool.size();
        image_base->push_back(o.texel_base);
        pool.insert(pool.end(), im.texels, im.texels + n_tex * im.channels);
    }
}

// MipMap::new's EWA weights (mipmap.rs:186-192), host expf like the reference's f32::exp
inline void ewa_weights(float lut[RSPT_EWA_LUT]) {
    for (int i = 0; i < RSPT_EWA_LUT; i++) {
        const float alpha = 2.0f, r2 = (float)i / (float)(RSPT_EWA_LUT - 1);
        lut[i] = std::exp(-alpha * r2) - std::exp(-alpha);
    }
}

// Distribution1D::new (sampling.rs:24-49): c[0 .. n] = the normalised cdf of f[0 .. n); returns the function's integral
inline float dist1d(const float* f, uint32_t n, float* c) {
    c[0] = 0.0f;
    for (uint32_t k = 1; k <= n; k++) c[k] = c[k - 1] + f[k - 1] / (float)n;
    float fi = c[n];
    if (fi == 0.0f) for (uint32_t k = 1; k <= n; k++) c[k] = (float)k / (float)n;
    else for (uint32_t k = 1; k <= n; k++) c[k] /= fi;
    return fi;
}
// Distribution2D::new (sampling.rs:156-170) = Distribution1D::new per row and for the marginal
struct EnvDist {
    std::vector<float> cdf, fint, mcdf;   // [nv][nu + 1] conditional cdfs, [nv] row integrals (the marginal's function), [nv + 1] marginal cdf
    float marg_int = 0.0f;
};
inline EnvDist build_env_dist(const rspt_envmap& e) {
    const uint32_t nu = e.dist_nu, nv = e.dist_nv;
    EnvDist out;
    out.cdf.resize((size_t)nv * (nu + 1)); out.fint.resize(nv); out.mcdf.resize(nv + 1);
    for (uint32_t v = 0; v < nv; v++) out.fint[v] = dist1d(e.dist_func + (size_t)v * nu, nu, out.cdf.data() + (size_t)v * (nu + 1));
    out.marg_int = dist1d(out.fint.data(), nv, out.mcdf.data());
    return out;
}

// Scene.infinite_lights (scene.rs:40-43)
inline std::vector<uint32_t> infinite_lights(const rspt_scene_desc* d) {
    std::vector<uint32_t> inf;
    for (uint32_t i = 0; i < d->n_lights; i++)
        if (d->lights[i].kind == RSPT_LIGHT_INFINITE) inf.push_back(i);
    return inf;
}

// 1 / max(density) of a grid medium (GridDensityMedium::new, grid.rs:44-55)
inline float grid_inv_max_density(const rspt_medium& m) {
    const size_t n = (size_t)m.nx * m.ny * m.nz;
    float max_density = 0.0f;
    for (size_t k = 0; k < n; k++) max_density = std::fmax(max_density, m.density[k]);   // f32::max
    return 1.0f / max_density;
}

// ---- primitives ----
// ABI 27: on the device a disk or cylinder primitive is a sphere primitive whose index names its slot behind the triangle records (dev_quadric.h: spheres, disks, cylinders)
inline std::vector<rspt_prim> quadric_prims_as_sphere_slots(const rspt_scene_desc* d) {
    std::vector<rspt_prim> pv(d->prims, d->prims + d->n_prims);
    for (rspt_prim& p : pv) {
        if (p.mesh == RSPT_MESH_DISK) { p.mesh = RSPT_MESH_SPHERE; p.v[0] += d->n_spheres; }
        else if (p.mesh == RSPT_MESH_CYLINDER) { p.mesh = RSPT_MESH_SPHERE; p.v[0] += d->n_spheres + d->n_disks; }
    }
    return pv;
}

// SceneDev::tri_nuv: every primitive's normals and uvs next to each other (80 B per primitive); wanted when some mesh has either
inline bool wants_tri_nuv(const rspt_scene_desc* d) {
    bool any = false;
    for (uint32_t i = 0; i < d->n_meshes; i++) any = any || (d->meshes[i].has_n && d->N) || (d->meshes[i].has_uv && d->UV);
    return any && d->n_prims;
}
inline std::vector<float> pack_tri_nuv(const rspt_scene_desc* d) {
    std::vector<float> nuv((size_t)d->n_prims * 20, 0.0f);
    for (uint64_t i = 0; i < d->n_prims; i++) {
        const rspt_prim& pr = d->prims[i];
        if (pr.mesh == RSPT_MESH_INSTANCE || pr.mesh == RSPT_MESH_SPHERE || pr.mesh == RSPT_MESH_DISK || pr.mesh == RSPT_MESH_CYLINDER) continue;
        const rspt_mesh& me = d->meshes[pr.mesh];
        float* q = nuv.data() + 20 * i;
        for (int k = 0; k < 3; k++) {
            if (me.has_n && d->N) for (int c = 0; c < 3; c++) q[3 * k + c] = d->N[3 * (size_t)pr.v[k] + c];
            if (me.has_uv && d->UV) for (int c = 0; c < 2; c++) q[9 + 2 * k + c] = d->UV[2 * (size_t)pr.v[k] + c];
        }
    }
    return nuv;
}

// ABI 23: the sphere records behind the primitive records (dev_sphere.h SphereDev)
inline std::vector<SphereDev> sphere_slots(const rspt_scene_desc* d) {
    std::vector<SphereDev> sph(d->n_spheres);
    memset(sph.data(), 0, sph.size() * sizeof(SphereDev));
    for (uint32_t k = 0; k < d->n_spheres; k++) sph[k].s = d->spheres[k];
    return sph;
}
// ABI 27: every slot with its kind — the spheres (kind 0), then the disks, then the cylinders
inline std::vector<QuadricDev> quadric_slots(const rspt_scene_desc* d) {
    std::vector<QuadricDev> q((size_t)d->n_spheres + d->n_disks + d->n_cylinders);
    memset(q.data(), 0, q.size() * sizeof(QuadricDev));
    for (uint32_t k = 0; k < d->n_spheres; k++) { q[k].s = d->spheres[k]; q[k].kind = QK_SPHERE; }
    for (uint32_t k = 0; k < d->n_disks; k++) { q[d->n_spheres + k].d = d->disks[k]; q[d->n_spheres + k].kind = QK_DISK; }
    for (uint32_t k = 0; k < d->n_cylinders; k++) { q[d->n_spheres + d->n_disks + k].c = d->cylinders[k]; q[d->n_spheres + d->n_disks + k].kind = QK_CYLINDER; }
    return q;
}

}  // namespace scene
}  // namespace rspt
