// The host side of rspt_scene_create, run without a GPU and under ASan / UBSan (tests/test_scene_host.py builds and runs this program):
//  (a) every refusal of scene_validate.h and of the texture-slot step, by code and full text, one changed field each, from one small valid scene;
//      scenes with two faults that pin which is reported first; the valid scene and every supported feature added to it pass;
//  (b) the records of scene_records.h held to invariants that follow from the structures alone (trace_w4.h, trace_w4q.h, trace_wide.h).
// One line per case; the first failure ends the program with a non-zero status.  No HIP runtime call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "scene_materials.h"
#include "scene_records.h"

using namespace rspt;
using namespace rspt::scene;

namespace {

int n_cases = 0;
[[noreturn]] void die(const std::string& name, const std::string& why) {
    printf("FAIL %s: %s\n", name.c_str(), why.c_str());
    fflush(stdout);
    exit(1);
}
void pass(const std::string& name) { printf("ok %s\n", name.c_str()); n_cases++; }
#define REQUIRE(name, cond) do { if (!(cond)) die(name, std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"); } while (0)

const float ID[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
const float NaN = __builtin_nanf(""), Inf = __builtin_huge_valf();

// a scene description that owns its arrays; patch: last-moment edits of the rspt_scene_desc itself (null pointers, counts)
struct Scene {
    std::vector<rspt_bvh_node> nodes;
    std::vector<rspt_prim> prims;
    std::vector<rspt_mesh> meshes;
    std::vector<float> P, UV;
    std::vector<rspt_material_desc> mats;
    std::vector<rspt_light> lights;
    std::vector<rspt_envmap> envs;
    std::vector<rspt_texture> texs;
    std::vector<rspt_image> imgs;
    std::vector<rspt_object> objs;
    std::vector<rspt_instance> insts;
    std::vector<rspt_medium> media;
    std::vector<rspt_sphere> spheres;
    std::vector<rspt_disk> disks;
    std::vector<rspt_cylinder> cyls;
    uint64_t n_top_nodes = 0, n_top_prims = 0;
    uint32_t mode = RSPT_INSTANCING_REFERENCE;
    std::function<void(rspt_scene_desc&)> patch;
    rspt_scene_desc desc() const {
        rspt_scene_desc d;
        memset(&d, 0, sizeof d);
        d.nodes = nodes.data(); d.n_nodes = nodes.size();
        d.prims = prims.data(); d.n_prims = prims.size();
        d.meshes = meshes.data(); d.n_meshes = (uint32_t)meshes.size();
        d.P = P.data(); d.UV = UV.empty() ? nullptr : UV.data(); d.n_vertices = P.size() / 3;
        d.materials = mats.data(); d.n_materials = (uint32_t)mats.size();
        d.lights = lights.data(); d.n_lights = (uint32_t)lights.size();
        d.envmaps = envs.data(); d.n_envmaps = (uint32_t)envs.size();
        d.textures = texs.data(); d.n_textures = (uint32_t)texs.size();
        d.images = imgs.data(); d.n_images = (uint32_t)imgs.size();
        d.objects = objs.data(); d.n_objects = (uint32_t)objs.size();
        d.instances = insts.data(); d.n_instances = (uint32_t)insts.size();
        d.n_top_nodes = n_top_nodes; d.n_top_prims = n_top_prims; d.instancing_mode = mode;
        d.media = media.data(); d.n_media = (uint32_t)media.size();
        d.spheres = spheres.data(); d.n_spheres = (uint32_t)spheres.size();
        d.disks = disks.data(); d.n_disks = (uint32_t)disks.size();
        d.cylinders = cyls.data(); d.n_cylinders = (uint32_t)cyls.size();
        if (patch) patch(d);
        return d;
    }
};

rspt_bvh_node leaf_node(int32_t first, uint16_t n, float x0, float x1) {
    rspt_bvh_node nd;
    memset(&nd, 0, sizeof nd);
    nd.bmin[0] = x0; nd.bmin[1] = -1.0f; nd.bmin[2] = -0.5f; nd.bmax[0] = x1; nd.bmax[1] = 1.0f; nd.bmax[2] = 0.25f;
    nd.offset = first; nd.n_prims = n;
    return nd;
}
rspt_bvh_node interior_node(int32_t second, uint8_t axis, float x0, float x1) {
    rspt_bvh_node nd = leaf_node(second, 0, x0, x1);
    nd.axis = axis;
    return nd;
}
rspt_texture constant_tex(float v) {
    rspt_texture t;
    memset(&t, 0, sizeof t);
    t.kind = RSPT_TEX_CONSTANT; t.value[0] = t.value[1] = t.value[2] = v;
    return t;
}
rspt_texture scale_tex(uint32_t a, uint32_t b) {
    rspt_texture t = constant_tex(0.0f);
    t.kind = RSPT_TEX_SCALE; t.tex1 = a; t.tex2 = b;
    return t;
}
rspt_texture checker_tex(uint32_t a, uint32_t b) {
    rspt_texture t = scale_tex(a, b);
    t.kind = RSPT_TEX_CHECKERBOARD; t.mapping = RSPT_MAP_UV; t.map[0] = t.map[1] = 1.0f;
    return t;
}
rspt_material_desc matte_mat(uint32_t kd_plus_1, uint32_t sigma_plus_1) {
    rspt_material_desc m;
    memset(&m, 0, sizeof m);
    m.kind = RSPT_MAT_MATTE; m.kd = kd_plus_1; m.sigma = sigma_plus_1; m.remap_roughness = 1;
    return m;
}
rspt_light area_light(uint32_t prim) {
    rspt_light l;
    memset(&l, 0, sizeof l);
    l.kind = RSPT_LIGHT_DIFFUSE_AREA; l.prim = prim; l.L[0] = l.L[1] = l.L[2] = 1.0f;
    return l;
}
rspt_prim tri_prim(uint32_t a, uint32_t b, uint32_t c, int32_t light = -1) { return rspt_prim{{a, b, c}, 0u, 0u, light}; }

// n triangles over the same four vertices, one matte material over two constant textures (0: grey, 1: sigma 0), no nodes yet
Scene scene_of_triangles(size_t n) {
    Scene s;
    s.P = {-1, -1, 0, 1, -1, 0, 1, 1, 0, -1, 1, 0};
    for (size_t i = 0; i < n; i++) s.prims.push_back(i % 2 ? tri_prim(0, 2, 3) : tri_prim(0, 1, 2));
    s.meshes.push_back(rspt_mesh{0, 0, 0, 0, 0, 0, 0, 0});
    s.texs = {constant_tex(0.5f), constant_tex(0.0f)};
    s.mats = {matte_mat(1, 2)};
    return s;
}
// the valid scene every refusal starts from: two triangles, a three-node BVH, one matte material, one area light (on primitive 0)
Scene base_scene() {
    Scene s = scene_of_triangles(2);
    s.nodes = {interior_node(2, 0, -1.0f, 1.0f), leaf_node(0, 1, -1.0f, 1.0f), leaf_node(1, 1, -1.0f, 0.5f)};
    s.prims[0].area_light = 0;
    s.lights = {area_light(0)};
    return s;
}
// a chain: every interior node's first child is a leaf of one primitive, its second child the next interior node; `levels` leaves deep
void append_chain(Scene& s, uint32_t levels, uint32_t first_prim) {
    const uint32_t base = (uint32_t)s.nodes.size();
    for (uint32_t k = 0; k + 1 < levels; k++) {
        s.nodes.push_back(interior_node((int32_t)(base + 2 * k + 2), (uint8_t)(k % 3), -1.0f - (float)k, 1.0f + 0.5f * (float)k));
        s.nodes.push_back(leaf_node((int32_t)(first_prim + k), 1, -1.0f - (float)k, 0.25f * (float)k));
    }
    s.nodes.push_back(leaf_node((int32_t)(first_prim + levels - 1), 1, -0.125f, 1.0f + 0.5f * (float)levels));
}
Scene chain_scene(uint32_t levels) {
    Scene s = scene_of_triangles(levels);
    append_chain(s, levels, 0);
    return s;
}
rspt_instance instance_of(uint32_t object) {
    rspt_instance in;
    memset(&in, 0, sizeof in);
    in.object = object;
    memcpy(in.to_world, ID, sizeof ID); memcpy(in.from_world, ID, sizeof ID);
    in.to_world[3] = 2.0f; in.from_world[3] = -2.0f;
    return in;
}
// two objects (a three-node aggregate of two triangles; a lone triangle), three instances; the top level is one leaf of four primitives:
// triangle, instance 0, instance 1 (in the middle of the leaf), instance 2
Scene instanced_scene() {
    Scene s = scene_of_triangles(7);
    for (uint32_t i = 0; i < 3; i++) {
        s.prims[1 + i] = rspt_prim{{i, 0, 0}, RSPT_MESH_INSTANCE, 0u, -1};
        s.insts.push_back(instance_of(i == 2 ? 1u : 0u));
    }
    s.nodes = {leaf_node(0, 4, -3.0f, 3.0f), interior_node(3, 1, -1.0f, 1.0f), leaf_node(4, 1, -1.0f, 0.0f), leaf_node(5, 1, 0.0f, 1.0f)};
    s.n_top_nodes = 1; s.n_top_prims = 4;
    s.objs = {rspt_object{1, 3, 4, 2}, rspt_object{0, 0, 6, 1}};
    return s;
}
rspt_sphere sphere_rec() {
    rspt_sphere sp;
    memset(&sp, 0, sizeof sp);
    memcpy(sp.object_to_world, ID, sizeof ID); memcpy(sp.world_to_object, ID, sizeof ID);
    sp.radius = 1.0f; sp.z_min = -1.0f; sp.z_max = 1.0f; sp.theta_min = 3.14159274f; sp.theta_max = 0.0f; sp.phi_max = 6.28318548f;
    return sp;
}
rspt_disk disk_rec() {
    rspt_disk k;
    memset(&k, 0, sizeof k);
    memcpy(k.object_to_world, ID, sizeof ID); memcpy(k.world_to_object, ID, sizeof ID);
    k.height = 0.0f; k.radius = 1.0f; k.inner_radius = 0.0f; k.phi_max = 6.28318548f;
    return k;
}
rspt_cylinder cylinder_rec() {
    rspt_cylinder k;
    memset(&k, 0, sizeof k);
    memcpy(k.object_to_world, ID, sizeof ID); memcpy(k.world_to_object, ID, sizeof ID);
    k.radius = 1.0f; k.z_min = -1.0f; k.z_max = 1.0f; k.phi_max = 6.28318548f;
    return k;
}
// the base scene with primitive 1 turned into an analytic shape
Scene shape_scene(uint32_t mesh) {
    Scene s = base_scene();
    s.spheres = {sphere_rec()}; s.disks = {disk_rec()}; s.cyls = {cylinder_rec()};
    if (mesh == RSPT_MESH_SPHERE) { s.disks.clear(); s.cyls.clear(); }
    s.prims[1] = rspt_prim{{0, 0, 0}, mesh, 0u, -1};
    return s;
}
rspt_medium homogeneous_medium() {
    rspt_medium m;
    memset(&m, 0, sizeof m);
    m.kind = RSPT_MEDIUM_HOMOGENEOUS;
    for (int c = 0; c < 3; c++) { m.sigma_a[c] = 0.5f; m.sigma_s[c] = 1.0f; }
    memcpy(m.world_to_medium, ID, sizeof ID);
    return m;
}
const float GRID_DENSITY[2] = {0.5f, 2.0f};
rspt_medium grid_medium() {
    rspt_medium m = homogeneous_medium();
    m.kind = RSPT_MEDIUM_GRID; m.nx = 2; m.ny = 1; m.nz = 1; m.density = GRID_DENSITY;
    return m;
}
rspt_light map_light(uint32_t kind) {
    rspt_light l = area_light(0xffffffffu);
    l.kind = kind;
    l.p[12] = l.p[13] = -1.0f; l.p[14] = l.p[15] = 1.0f;
    return l;
}
const float TEXELS_4x2[3 * 11] = {1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 1, 1, 1};
const float DIST_4x2[8] = {0.5f, 1.5f, 0.25f, 3.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // the second row takes Distribution1D's uniform branch
rspt_image image_4x2() { return rspt_image{4, 2, 3, 3, TEXELS_4x2}; }
rspt_envmap envmap_4x2() {
    rspt_envmap e;
    memset(&e, 0, sizeof e);
    e.width = 4; e.height = 2; e.n_levels = 3; e.texels = TEXELS_4x2; e.dist_nu = 4; e.dist_nv = 2; e.dist_func = DIST_4x2;
    return e;
}
rspt_light infinite_light(uint32_t envmap) {
    rspt_light l = area_light(envmap);
    l.kind = RSPT_LIGHT_INFINITE;
    return l;
}
rspt_texture image_tex(uint32_t image) {
    rspt_texture t = checker_tex(0, 0);
    t.kind = RSPT_TEX_IMAGE; t.image = image; t.max_aniso = 8.0f;
    return t;
}
// material 0 becomes a mix of two plastics whose Kd, Ks and roughness are six distinct checkerboards: more than RSPT_TEX_SLOTS
void bind_six_textures(Scene& s) {
    for (int k = 0; k < 6; k++) { rspt_texture t = checker_tex(0, 1); t.map[0] = 2.0f + (float)k; s.texs.push_back(t); }
    rspt_material_desc mix = matte_mat(0, 0), pl[2] = {matte_mat(3, 0), matte_mat(6, 0)};
    mix.kind = RSPT_MAT_MIX; mix.amount = 1; mix.m1 = 1; mix.m2 = 2;
    for (int k = 0; k < 2; k++) { pl[k].kind = RSPT_MAT_PLASTIC; pl[k].ks = pl[k].kd + 1; pl[k].roughness = pl[k].kd + 2; }
    s.mats = {mix, pl[0], pl[1]};
}

Error run(const Scene& s, SceneFacts* facts = nullptr, SceneMaterials* sm = nullptr) {
    SceneFacts f;
    SceneMaterials m;
    const rspt_scene_desc d = s.desc();
    return prepare_scene(&d, facts ? facts : &f, sm ? sm : &m);
}
void accepts(const std::string& name, const Scene& s) {
    const Error e = run(s);
    if (e) die(name, "refused: " + e.text);
    pass("accepts " + name);
}
void refuses(Scene s, int code, const std::string& text, const std::function<void(Scene&)>& change) {
    change(s);
    const Error e = run(s);
    if (e.code != code || e.text != text) die("refuses \"" + text + "\"", "got " + std::to_string(e.code) + " \"" + e.text + "\"");
    pass("refuses (" + std::to_string(code) + ") " + text);
}

const int INV = RSPT_E_INVALID, UNS = RSPT_E_UNSUPPORTED;
const unsigned NONE_MAT = 0xffffffffu;

void refusal_cases() {
    const Scene base = base_scene(), inst = instanced_scene();
    const Scene sph = shape_scene(RSPT_MESH_SPHERE), dsk = shape_scene(RSPT_MESH_DISK), cyl = shape_scene(RSPT_MESH_CYLINDER);
    // ---- arguments and counts ----
    {
        SceneFacts f; SceneMaterials m;
        const Error e = prepare_scene(nullptr, &f, &m);
        REQUIRE("null description", e.code == INV && e.text == "null argument");
        pass("refuses (-1) null argument");
    }
    refuses(base, UNS, "more than 2^31 primitives / nodes", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.n_prims = 0x80000000ull; }; });
    refuses(base, UNS, "more than 2^31 primitives / nodes", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.n_nodes = 0x80000000ull; }; });
    refuses(base, INV, "null array with non-zero count", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.nodes = nullptr; }; });
    refuses(base, INV, "null array with non-zero count", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.prims = nullptr; }; });
    refuses(base, INV, "null array with non-zero count", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.meshes = nullptr; }; });
    refuses(base, INV, "null array with non-zero count", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.P = nullptr; }; });
    refuses(base, INV, "null array with non-zero count", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.materials = nullptr; }; });
    refuses(base, INV, "null array with non-zero count", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.lights = nullptr; }; });
    refuses(base, INV, "nodes and prims must both be empty or both non-empty", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.n_nodes = 0; }; });
    // ---- instances and objects ----
    refuses(inst, UNS, "spheres together with object instances", [](Scene& s) { s.spheres = {sphere_rec()}; });
    refuses(inst, UNS, "disks together with object instances", [](Scene& s) { s.disks = {disk_rec()}; });
    refuses(inst, UNS, "cylinders together with object instances", [](Scene& s) { s.cyls = {cylinder_rec()}; });
    refuses(inst, INV, "instances without objects", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.objects = nullptr; }; });
    refuses(inst, INV, "instances without objects", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.n_objects = 0; }; });
    refuses(inst, INV, "bad top-level aggregate range", [](Scene& s) { s.n_top_nodes = 0; });
    refuses(inst, INV, "bad top-level aggregate range", [](Scene& s) { s.n_top_prims = 8; });
    refuses(inst, INV, "bad instancing_mode", [](Scene& s) { s.mode = 7; });
    refuses(inst, INV, "object 0: primitive range", [](Scene& s) { s.objs[0].n_prims = 0; });
    refuses(inst, INV, "object 1: primitive range", [](Scene& s) { s.objs[1].first_prim = 3; });
    refuses(inst, INV, "object 0: node range", [](Scene& s) { s.objs[0].first_node = 0; });
    refuses(inst, INV, "object 1: node range", [](Scene& s) { s.objs[1].n_prims = 2; s.objs[1].first_prim = 5; });
    refuses(inst, INV, "instance 2: object index out of range", [](Scene& s) { s.insts[2].object = 2; });
    refuses(inst, INV, "instance 1: non-finite transform", [](Scene& s) { s.insts[1].to_world[15] = NaN; });
    refuses(inst, INV, "instance 1: non-finite transform", [](Scene& s) { s.insts[1].from_world[0] = Inf; });
    // ---- spheres, disks, cylinders ----
    refuses(sph, INV, "null spheres with n_spheres > 0", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.spheres = nullptr; }; });
    refuses(sph, INV, "sphere 0: non-finite transform", [](Scene& s) { s.spheres[0].world_to_object[7] = NaN; });
    refuses(sph, INV, "sphere 0: radius must be positive and finite, z / theta / phi finite", [](Scene& s) { s.spheres[0].radius = 0.0f; });
    refuses(sph, INV, "sphere 0: radius must be positive and finite, z / theta / phi finite", [](Scene& s) { s.spheres[0].theta_max = Inf; });
    refuses(sph, INV, "sphere 0: medium index out of range", [](Scene& s) { s.spheres[0].medium_inside = 1; });
    refuses(dsk, INV, "null disks with n_disks > 0", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.disks = nullptr; }; });
    refuses(dsk, INV, "null cylinders with n_cylinders > 0", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.cylinders = nullptr; }; });
    refuses(dsk, UNS, "more than 2^31 spheres, disks and cylinders", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.n_spheres = 0; d.n_disks = d.n_cylinders = 0x40000000u; }; });
    refuses(dsk, INV, "disk 0: non-finite transform", [](Scene& s) { s.disks[0].object_to_world[0] = Inf; });
    refuses(dsk, INV, "disk 0: non-finite parameter", [](Scene& s) { s.disks[0].height = NaN; });
    refuses(dsk, INV, "disk 0: radius must be positive", [](Scene& s) { s.disks[0].radius = -1.0f; });
    refuses(dsk, INV, "disk 0: radius equals inner_radius (v divides by their difference)", [](Scene& s) { s.disks[0].inner_radius = 1.0f; });
    refuses(dsk, INV, "disk 0: phi_max outside (0, 2 pi]", [](Scene& s) { s.disks[0].phi_max = 0.0f; });
    refuses(dsk, INV, "disk 0: phi_max outside (0, 2 pi]", [](Scene& s) { s.disks[0].phi_max = 6.2831864f; });
    refuses(dsk, INV, "disk 0: medium index out of range", [](Scene& s) { s.disks[0].medium_outside = 1; });
    refuses(cyl, INV, "cylinder 0: non-finite transform", [](Scene& s) { s.cyls[0].world_to_object[15] = NaN; });
    refuses(cyl, INV, "cylinder 0: non-finite parameter", [](Scene& s) { s.cyls[0].z_max = Inf; });
    refuses(cyl, INV, "cylinder 0: radius must be positive", [](Scene& s) { s.cyls[0].radius = 0.0f; });
    refuses(cyl, INV, "cylinder 0: z_min equals z_max (v divides by their difference)", [](Scene& s) { s.cyls[0].z_min = 1.0f; });
    refuses(cyl, INV, "cylinder 0: phi_max outside (0, 2 pi]", [](Scene& s) { s.cyls[0].phi_max = -1.0f; });
    refuses(cyl, INV, "cylinder 0: medium index out of range", [](Scene& s) { s.cyls[0].medium_inside = 2; });
    // ---- primitives ----
    const Scene* shapes[3] = {&sph, &dsk, &cyl};
    const char* kn[3] = {"sphere", "disk", "cylinder"};
    for (int k = 0; k < 3; k++) {
        const std::string n = kn[k];
        refuses(*shapes[k], INV, "prim 1: " + n + " index out of range", [](Scene& s) { s.prims[1].v[0] = 1; });
        refuses(*shapes[k], INV, k == 0 ? std::string("prim 1: material index out of range") : "prim 1: " + n + "'s material index out of range", [](Scene& s) { s.prims[1].material = 1; });
        refuses(*shapes[k], INV, "prim 1: " + n + "'s light index out of range", [](Scene& s) { s.prims[1].area_light = -2; });
        refuses(*shapes[k], INV, "prim 1: " + n + "'s light index out of range", [](Scene& s) { s.prims[1].area_light = 1; });
        refuses(*shapes[k], INV, "prim 1: " + n + "'s area light 0 is not a DIFFUSE_AREA light on this primitive", [](Scene& s) { s.prims[1].area_light = 0; });
        refuses(*shapes[k], INV, "prim 1: " + n + "'s area light 1 is not a DIFFUSE_AREA light on this primitive", [](Scene& s) { s.prims[1].area_light = 1; s.lights.push_back(map_light(RSPT_LIGHT_POINT)); });
        refuses(*shapes[k], INV, "light 1: its " + n + " primitive names another light", [](Scene& s) { s.lights.push_back(area_light(1)); });
    }
    refuses(base, INV, "prim 1: bad instance reference", [](Scene& s) { s.prims[1].mesh = RSPT_MESH_INSTANCE; });
    refuses(inst, INV, "prim 4: bad instance reference", [](Scene& s) { s.prims[4].mesh = RSPT_MESH_INSTANCE; });
    refuses(inst, INV, "prim 2: bad instance reference", [](Scene& s) { s.prims[2].v[0] = 3; });
    refuses(inst, UNS, "prim 5: area lights are not supported with object instancing (api.rs:2899)", [](Scene& s) { s.prims[5].area_light = 0; s.lights = {area_light(0)}; });
    refuses(base, INV, "prim 1: vertex index out of range", [](Scene& s) { s.prims[1].v[2] = 4; });
    refuses(base, INV, "prim 1: mesh index out of range", [](Scene& s) { s.prims[1].mesh = 1; });
    refuses(base, INV, "prim 1: material index out of range", [](Scene& s) { s.prims[1].material = 1; });
    refuses(base, INV, "prim 1: light index out of range", [](Scene& s) { s.prims[1].area_light = 1; });
    // ---- meshes, media, emissive meshes with alpha ----
    refuses(base, INV, "mesh 0: alpha texture index out of range", [](Scene& s) { s.meshes[0].shadow_alpha_tex = 3; });
    refuses(base, INV, "mesh 0: medium index out of range", [](Scene& s) { s.meshes[0].medium_inside = 1; });
    refuses(base, INV, "null media", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.n_media = 1; d.media = nullptr; }; });
    refuses(base, UNS, "medium 0: kind 9 (homogeneous and grid-density media)", [](Scene& s) { s.media = {homogeneous_medium()}; s.media[0].kind = 9; });
    refuses(base, INV, "medium 0: bad density grid", [](Scene& s) { s.media = {grid_medium()}; s.media[0].ny = 0; });
    refuses(base, INV, "medium 0: bad density grid", [](Scene& s) { s.media = {grid_medium()}; s.media[0].density = nullptr; });
    refuses(base, UNS, "medium 0: projective world_to_medium", [](Scene& s) { s.media = {grid_medium()}; s.media[0].world_to_medium[12] = 0.5f; });
    refuses(base, INV, "medium 1: bad sigma_a / sigma_s", [](Scene& s) { s.media = {grid_medium(), homogeneous_medium()}; s.media[1].sigma_s[2] = -0.5f; });
    refuses(base, INV, "medium 0: bad sigma_a / sigma_s", [](Scene& s) { s.media = {homogeneous_medium()}; s.media[0].sigma_a[0] = Inf; });
    refuses(base, INV, "medium 0: g outside (-1, 1)", [](Scene& s) { s.media = {homogeneous_medium()}; s.media[0].g = 1.0f; });
    refuses(base, UNS, "prim 0: an emissive mesh with an alpha mask", [](Scene& s) { s.meshes[0].alpha_tex = 1; });
    // ---- lights ----
    refuses(base, UNS, "light 0: unsupported kind 0", [](Scene& s) { s.lights[0].kind = 0; });
    refuses(base, UNS, "light 0: unsupported kind 8", [](Scene& s) { s.lights[0].kind = 8; });
    refuses(base, INV, "light 0: prim out of range", [](Scene& s) { s.lights[0].prim = 2; });
    refuses(inst, INV, "light 0: prim out of range", [](Scene& s) { s.lights = {area_light(1)}; });   // an instance primitive
    refuses(base, INV, "light 1: envmap index out of range", [](Scene& s) { s.lights.push_back(infinite_light(0)); });
    refuses(base, INV, "light 1 (projection): non-finite intensity", [](Scene& s) { s.lights.push_back(map_light(RSPT_LIGHT_PROJECTION)); s.lights[1].L[2] = NaN; });
    refuses(base, INV, "light 1 (goniometric): non-finite intensity", [](Scene& s) { s.lights.push_back(map_light(RSPT_LIGHT_GONIOMETRIC)); s.lights[1].L[0] = Inf; });
    refuses(base, INV, "light 1 (projection): non-finite parameter p[21]", [](Scene& s) { s.lights.push_back(map_light(RSPT_LIGHT_PROJECTION)); s.lights[1].p[21] = NaN; });
    refuses(base, INV, "light 1 (goniometric): non-finite parameter p[11]", [](Scene& s) { s.lights.push_back(map_light(RSPT_LIGHT_GONIOMETRIC)); s.lights[1].p[11] = NaN; });
    refuses(base, INV, "light 1 (projection): map index out of range", [](Scene& s) { s.lights.push_back(map_light(RSPT_LIGHT_PROJECTION)); s.lights[1].prim = 0; });
    refuses(base, INV, "light 1 (goniometric): map index out of range", [](Scene& s) { s.lights.push_back(map_light(RSPT_LIGHT_GONIOMETRIC)); s.lights[1].prim = 0; });
    refuses(base, INV, "light 1 (projection): screen_bounds min above max", [](Scene& s) { s.lights.push_back(map_light(RSPT_LIGHT_PROJECTION)); s.lights[1].p[13] = 2.0f; });
    // ---- images and the texture graph ----
    refuses(base, INV, "null texture / image array", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.n_images = 1; d.images = nullptr; }; });
    refuses(base, INV, "null texture / image array", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.textures = nullptr; }; });
    refuses(base, INV, "image 0: sides must be powers of two <= 32768 (MipMap::new resamples first)", [](Scene& s) { s.imgs = {image_4x2()}; s.imgs[0].width = 3; });
    refuses(base, INV, "image 0: sides must be powers of two <= 32768 (MipMap::new resamples first)", [](Scene& s) { s.imgs = {image_4x2()}; s.imgs[0].height = 65536; });
    refuses(base, INV, "image 0: n_levels 5, expected 3", [](Scene& s) { s.imgs = {image_4x2()}; s.imgs[0].n_levels = 5; });
    refuses(base, INV, "image 0: null texels or channels not 1 / 3", [](Scene& s) { s.imgs = {image_4x2()}; s.imgs[0].channels = 2; });
    refuses(base, INV, "image 0: null texels or channels not 1 / 3", [](Scene& s) { s.imgs = {image_4x2()}; s.imgs[0].texels = nullptr; });
    refuses(base, UNS, "texture 2: unsupported kind 0", [](Scene& s) { s.texs.push_back(constant_tex(1.0f)); s.texs[2].kind = 0; });
    refuses(base, UNS, "texture 2: unsupported kind 11", [](Scene& s) { s.texs.push_back(constant_tex(1.0f)); s.texs[2].kind = 11; });
    refuses(base, UNS, "texture 2: 2-D mapping 5", [](Scene& s) { s.texs.push_back(checker_tex(0, 1)); s.texs[2].mapping = RSPT_MAP_IDENTITY3D; });
    refuses(base, UNS, "texture 2: 3-D textures take the identity mapping", [](Scene& s) { s.texs.push_back(checker_tex(0, 1)); s.texs[2].kind = RSPT_TEX_FBM; });
    refuses(base, INV, "texture 2: octaves out of range", [](Scene& s) { s.texs.push_back(checker_tex(0, 1)); s.texs[2].kind = RSPT_TEX_MARBLE; s.texs[2].mapping = RSPT_MAP_IDENTITY3D; s.texs[2].octaves = 65; });
    refuses(base, INV, "texture 2: image index out of range", [](Scene& s) { s.texs.push_back(image_tex(0)); });
    refuses(base, INV, "texture 2: bad wrap mode", [](Scene& s) { s.imgs = {image_4x2()}; s.texs.push_back(image_tex(0)); s.texs[2].wrap = 3; });
    refuses(base, INV, "texture 2: child index out of range or cyclic graph", [](Scene& s) { s.texs.push_back(scale_tex(0, 3)); });
    refuses(base, INV, "texture 2: child index out of range or cyclic graph", [](Scene& s) { s.texs.push_back(scale_tex(3, 0)); s.texs.push_back(scale_tex(1, 2)); });
    refuses(base, UNS, "texture 4: graph deeper than 3 levels", [](Scene& s) { s.texs.push_back(scale_tex(0, 1)); s.texs.push_back(scale_tex(1, 2)); s.texs.push_back(scale_tex(3, 0)); });
    // ---- the material assembly's own refusals pass through ----
    refuses(base, UNS, "material 0: material kind 12 (matte, plastic, mirror, glass, metal, substrate, uber, translucent, mix)", [](Scene& s) { s.mats[0].kind = 12; });
    // ---- envmaps ----
    refuses(base, INV, "null envmaps", [](Scene& s) { s.patch = [](rspt_scene_desc& d) { d.n_envmaps = 1; d.envmaps = nullptr; }; });
    refuses(base, INV, "envmap 0: sides must be powers of two <= 32768", [](Scene& s) { s.envs = {envmap_4x2()}; s.envs[0].height = 6; });
    refuses(base, INV, "envmap 0: n_levels 1, expected 3", [](Scene& s) { s.envs = {envmap_4x2()}; s.envs[0].n_levels = 1; });
    refuses(base, INV, "envmap 0: null data", [](Scene& s) { s.envs = {envmap_4x2()}; s.envs[0].texels = nullptr; });
    refuses(base, INV, "envmap 0: null data", [](Scene& s) { s.envs = {envmap_4x2()}; s.envs[0].dist_func = nullptr; s.lights.push_back(infinite_light(0)); s.lights.push_back(map_light(RSPT_LIGHT_GONIOMETRIC)); s.lights[2].prim = 0; });
    refuses(base, INV, "envmap 0: null data", [](Scene& s) { s.envs = {envmap_4x2()}; s.envs[0].dist_func = nullptr; });   // no distribution, yet no map light names it
    // ---- BVH shape and depth ----
    refuses(base, INV, "BVH is not a tree", [](Scene& s) { s.nodes[1] = interior_node(2, 0, -1.0f, 1.0f); });
    refuses(base, INV, "node 2: leaf range out of bounds", [](Scene& s) { s.nodes[2].offset = 2; });
    refuses(base, INV, "node 1: leaf range out of bounds", [](Scene& s) { s.nodes[1].offset = -1; });
    refuses(base, INV, "node 0: bad children", [](Scene& s) { s.nodes[0].axis = 3; });
    refuses(base, INV, "node 0: bad children", [](Scene& s) { s.nodes[0].offset = 3; });
    refuses(chain_scene(65), UNS, "BVH deeper than the 64-entry traversal stack", [](Scene&) {});
    refuses(inst, INV, "object 0: node 1: bad children", [](Scene& s) { s.nodes[1].offset = 1; });
    refuses(inst, INV, "object 0: node 3: leaf range out of bounds", [](Scene& s) { s.nodes[3].offset = 6; });
    {   // a top-level chain of 40 levels whose last primitive is an instance of a chain of 30 levels
        Scene s = scene_of_triangles(70);
        append_chain(s, 40, 0);
        s.n_top_nodes = s.nodes.size(); s.n_top_prims = 40;
        append_chain(s, 30, 40);
        s.prims[39] = rspt_prim{{0, 0, 0}, RSPT_MESH_INSTANCE, 0u, -1};
        s.insts = {instance_of(0)};
        s.objs = {rspt_object{s.n_top_nodes, 59, 40, 30}};
        refuses(s, UNS, "top-level BVH (40 levels) + object BVH (30 levels) deeper than the 64-entry traversal stack", [](Scene&) {});
        s.objs[0] = rspt_object{s.n_top_nodes + 12, 47, 46, 24};   // the chain's lower 24 levels: 64 in all
        accepts("a top-level BVH of 40 levels over an object BVH of 24", s);
    }
    // ---- texture slots ----
    refuses(base, UNS, "material 0 binds more than 4 distinct textures", bind_six_textures);
    // ---- moving instances ----
    auto moving = [](Scene& s) { s.insts[1].animated = 1; memcpy(s.insts[1].to_world_end, ID, sizeof ID); memcpy(s.insts[1].from_world_end, ID, sizeof ID); s.insts[1].time[1] = 1.0f; };
    refuses(inst, INV, "instance 1: animated with time[1] <= time[0] or a non-finite key time", [&](Scene& s) { moving(s); s.insts[1].time[0] = 1.0f; });
    refuses(inst, INV, "instance 1: animated with time[1] <= time[0] or a non-finite key time", [&](Scene& s) { moving(s); s.insts[1].time[1] = Inf; });
    refuses(inst, INV, "instance 1: non-finite end key matrix", [&](Scene& s) { moving(s); s.insts[1].from_world_end[5] = NaN; });
    refuses(inst, INV, "instance 1: end key with a zero homogeneous row", [&](Scene& s) { moving(s); s.insts[1].to_world_end[15] = 0.0f; });
    refuses(inst, INV, "instance 1: end key inverse with a zero homogeneous row", [&](Scene& s) { moving(s); s.insts[1].from_world_end[15] = 0.0f; });

    // ---- two faults: which one is reported ----
    refuses(sph, INV, "sphere 0: radius must be positive and finite, z / theta / phi finite", [](Scene& s) { s.spheres[0].radius = -1.0f; s.prims[0].v[0] = 9; });
    refuses(base, INV, "prim 0: vertex index out of range", [](Scene& s) { s.prims[0].v[0] = 9; s.meshes[0].medium_inside = 1; });
    refuses(base, INV, "mesh 0: medium index out of range", [](Scene& s) { s.meshes[0].medium_inside = 2; s.media = {homogeneous_medium()}; s.media[0].g = 2.0f; });
    refuses(base, INV, "light 0: prim out of range", [](Scene& s) { s.lights[0].prim = 2; s.texs.push_back(scale_tex(0, 9)); });
    refuses(base, INV, "texture 2: child index out of range or cyclic graph", [](Scene& s) { s.texs.push_back(scale_tex(0, 9)); s.envs = {envmap_4x2()}; s.envs[0].width = 5; });
    refuses(base, INV, "texture 2: child index out of range or cyclic graph", [](Scene& s) { s.texs.push_back(scale_tex(0, 9)); s.mats[0].kind = 12; });
    refuses(base, UNS, "material 0: material kind 12 (matte, plastic, mirror, glass, metal, substrate, uber, translucent, mix)", [](Scene& s) { s.mats[0].kind = 12; s.envs = {envmap_4x2()}; s.envs[0].width = 5; });
    refuses(base, INV, "envmap 0: sides must be powers of two <= 32768", [](Scene& s) { s.envs = {envmap_4x2()}; s.envs[0].width = 5; s.nodes[0].axis = 3; });
    refuses(base, INV, "envmap 0: sides must be powers of two <= 32768", [](Scene& s) { bind_six_textures(s); s.envs = {envmap_4x2()}; s.envs[0].width = 5; });
    refuses(base, INV, "node 0: bad children", [](Scene& s) { bind_six_textures(s); s.nodes[0].axis = 3; });
    refuses(inst, UNS, "material 0 binds more than 4 distinct textures", [&](Scene& s) { bind_six_textures(s); moving(s); s.insts[1].time[1] = -1.0f; });
    refuses(inst, INV, "instance 0: non-finite transform", [&](Scene& s) { s.insts[0].to_world[0] = NaN; moving(s); s.insts[1].time[1] = -1.0f; });

    // ---- what is served passes ----
    accepts("the base scene", base);
    accepts("an empty scene", Scene());
    accepts("a sphere", sph);
    accepts("a disk", dsk);
    accepts("a cylinder", cyl);
    { Scene s = sph; s.prims[1].area_light = 1; s.lights.push_back(area_light(1)); accepts("an emissive sphere", s); }
    { Scene s = dsk; s.prims[1].area_light = 1; s.lights.push_back(area_light(1)); SceneFacts f; REQUIRE("emissive disk", !run(s, &f) && f.disk_light && !f.cylinder_light); pass("accepts an emissive disk"); }
    { Scene s = cyl; s.prims[1].area_light = 1; s.lights.push_back(area_light(1)); SceneFacts f; REQUIRE("emissive cylinder", !run(s, &f) && f.cylinder_light && !f.disk_light); pass("accepts an emissive cylinder"); }
    accepts("object instances", inst);
    { Scene s = inst; s.mode = RSPT_INSTANCING_FIXED; moving(s); s.insts[1].to_world_end[3] = 5.0f; accepts("a moving instance", s); }
    { Scene s = base; s.media = {homogeneous_medium(), grid_medium()}; s.meshes[0].medium_inside = 2; s.meshes[0].medium_outside = 1; accepts("homogeneous and grid media", s); }
    {
        Scene s = base;
        s.meshes.push_back(s.meshes[0]); s.meshes[1].alpha_tex = 1; s.meshes[1].shadow_alpha_tex = 2; s.prims[1].mesh = 1;
        SceneFacts f;
        REQUIRE("alpha mask", !run(s, &f) && f.any_alpha);
        pass("accepts an alpha-masked mesh beside an emissive one");
    }
    { Scene s = base; s.prims[1].material = NONE_MAT; SceneFacts f; REQUIRE("null material", !run(s, &f) && f.has_null); pass("accepts a primitive without material"); }
    {
        Scene s = base;
        s.envs = {envmap_4x2(), envmap_4x2()}; s.envs[1].dist_func = nullptr; s.envs[1].dist_nu = s.envs[1].dist_nv = 0;
        s.lights.push_back(infinite_light(0)); s.lights.push_back(map_light(RSPT_LIGHT_PROJECTION)); s.lights.push_back(map_light(RSPT_LIGHT_GONIOMETRIC)); s.lights[3].prim = 1;
        for (uint32_t k : {RSPT_LIGHT_POINT, RSPT_LIGHT_SPOT, RSPT_LIGHT_DISTANT}) s.lights.push_back(map_light(k));
        SceneFacts f;
        SceneMaterials m;
        REQUIRE("lights", !run(s, &f, &m) && f.has_maplights && f.has_projection && f.has_goniometric);
        REQUIRE("lights", (m.shade_features & (SF_L_AREA | SF_L_POINT | SF_L_SPOT | SF_L_DISTANT | SF_L_INFINITE | SF_L_MAP)) == (SF_L_AREA | SF_L_POINT | SF_L_SPOT | SF_L_DISTANT | SF_L_INFINITE | SF_L_MAP));
        pass("accepts every light kind, an envmap with and one without a distribution");
    }
    {
        Scene s = base;
        s.UV = {0, 0, 1, 0, 1, 1, 0, 1}; s.meshes[0].has_uv = 1;
        s.imgs = {image_4x2()};
        s.texs.push_back(image_tex(0)); s.texs.push_back(checker_tex(2, 0)); s.texs.push_back(scale_tex(3, 1));   // three levels deep
        s.mats[0].kd = 5;
        SceneMaterials m;
        REQUIRE("textured", !run(s, nullptr, &m) && m.textured[0] && m.textured[1] && (m.shade_features & SF_TEX) && (m.shade_features & SF_VERTEX));
        REQUIRE("textured", m.bxdfs[0].size() == 1 && m.bxdfs[0][0].tex_r == 1u && m.slots[0][0] == 4u && m.slots[0][1] == 0xffffffffu && m.mflags[0][0] == RSPT_MAT_TEXTURED);
        pass("accepts an image texture under a three-level graph; Kd takes slot 1");
    }
    {   // four distinct textures fit
        Scene s = base;
        bind_six_textures(s);
        s.mats[2].roughness = 1;   // (a constant)
        SceneMaterials m;
        const Error e = run(s, nullptr, &m);
        REQUIRE("five slots", e.code == UNS && e.text == "material 0 binds more than 4 distinct textures");
        s.mats[1].roughness = 1;
        SceneMaterials m4;
        REQUIRE("four slots", !run(s, nullptr, &m4));
        for (int k = 0; k < 4; k++) REQUIRE("four slots", m4.slots[0][k] != 0xffffffffu);
        pass("accepts a mix binding exactly four textures, refuses five");
    }
}

// =====================================================================================================================================
// (b) record invariants
// =====================================================================================================================================
uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
bool same_bits(float a, float b) { return bits(a) == bits(b); }

struct Walk {
    std::string name;
    const rspt_scene_desc* d;
    const SceneFacts* f;
    const W4Records* w;
    std::vector<uint32_t> seen;   // per primitive: times reached
    size_t n_records = 0;         // records walked
    // (first, count) of a leaf reference
    std::pair<uint32_t, uint32_t> range(uint32_t ref) const {
        REQUIRE(name, ref & RSPT_REF_LEAF);
        const uint32_t cnt = (ref >> RSPT_W4_COUNT_SHIFT) & 15u, low = ref & RSPT_W4_OFFSET_MASK;
        if (cnt < 15u) return {low, cnt + 1u};
        REQUIRE(name, low < w->big_leaves.size());
        return {w->big_leaves[low].x, w->big_leaves[low].y};
    }
    void leaf(uint32_t ref, uint32_t node) {
        const rspt_bvh_node& n = d->nodes[node];
        const auto r = range(ref);
        REQUIRE(name, r.first == (uint32_t)n.offset && r.second == n.n_prims);
        REQUIRE(name, (n.n_prims > 15u) == (((ref >> RSPT_W4_COUNT_SHIFT) & 15u) == 15u));
        for (uint32_t i = 0; i < n.n_prims; i++) seen[r.first + i]++;
    }
    // record `ri` against the interior LinearBVHNode `a`
    void record(uint32_t ri, uint32_t a) {
        REQUIRE(name, ri < w->recs.size());
        n_records++;
        const Wide4Node& rec = w->recs[ri];
        const rspt_bvh_node& A = d->nodes[a];
        REQUIRE(name, A.n_prims == 0);
        uint32_t slot[4] = {RSPT_NONE, RSPT_NONE, RSPT_NONE, RSPT_NONE}, axes[3] = {A.axis, 0u, 0u};
        const uint32_t child[2] = {a + 1u, (uint32_t)A.offset};
        for (int g = 0; g < 2; g++) {
            const rspt_bvh_node& c = d->nodes[child[g]];
            if (c.n_prims) slot[2 * g] = child[g];
            else { slot[2 * g] = child[g] + 1u; slot[2 * g + 1] = (uint32_t)c.offset; axes[1 + g] = c.axis; }
        }
        for (int k = 0; k < 3; k++) REQUIRE(name, ((rec.ref[k] & RSPT_W4_AXIS_MASK) >> RSPT_W4_AXIS_SHIFT) == axes[k]);
        for (int k = 0; k < 4; k++) {
            const float4* b = rec.b + (k < 2 ? 0 : 3);
            const float lo[3] = {k & 1 ? b[0].y : b[0].x, k & 1 ? b[1].y : b[1].x, k & 1 ? b[2].y : b[2].x};
            const float hi[3] = {k & 1 ? b[0].w : b[0].z, k & 1 ? b[1].w : b[1].z, k & 1 ? b[2].w : b[2].z};
            const uint32_t ref = k < 3 ? (rec.ref[k] & ~RSPT_W4_AXIS_MASK) : rec.ref[k];
            if (slot[k] == RSPT_NONE) {
                for (int c = 0; c < 3; c++) REQUIRE(name, lo[c] != lo[c] && hi[c] != hi[c]);
                REQUIRE(name, (rec.ref[k] | (k < 3 ? RSPT_W4_AXIS_MASK : 0u)) == RSPT_NONE);
                continue;
            }
            const rspt_bvh_node& x = d->nodes[slot[k]];
            for (int c = 0; c < 3; c++) REQUIRE(name, same_bits(lo[c], x.bmin[c]) && same_bits(hi[c], x.bmax[c]));
            if (x.n_prims) { leaf(ref, slot[k]); continue; }
            REQUIRE(name, !(ref & RSPT_REF_LEAF) && ref < w->recs.size() && ref != ri);
            if (ref < w->w4_top) REQUIRE(name, ri < ref);   // a record of the breadth-first prefix follows its parent
            record(ref, slot[k]);
        }
    }
    void tree(uint32_t root_ref, uint32_t root_node) {
        if (d->nodes[root_node].n_prims) leaf(root_ref, root_node);
        else { REQUIRE(name, !(root_ref & RSPT_REF_LEAF)); record(root_ref, root_node); }
    }
};

void check_quad4(const std::string& name, const std::vector<Wide4Node>& recs) {
    std::vector<Quad4Node> q;
    REQUIRE(name, quantise_w4(recs, &q) && q.size() == recs.size());
    for (size_t i = 0; i < recs.size(); i++) {
        const Wide4Node& w = recs[i];
        const Quad4Node& o = q[i];
        REQUIRE(name, !memcmp(o.ref, w.ref, sizeof o.ref));
        const uint32_t qlo[3] = {o.qlo[0], o.qlo[1], o.qlo[2]}, qhi[3] = {o.qhi_x, o.qhi_y, o.qhi_z};
        for (int c = 0; c < 3; c++) {
            const float lo4[4] = {w.b[c].x, w.b[c].y, w.b[3 + c].x, w.b[3 + c].y}, hi4[4] = {w.b[c].z, w.b[c].w, w.b[3 + c].z, w.b[3 + c].w};
            const int e = (int)((o.meta >> (8 * c)) & 255u);
            const double cell = std::ldexp(1.0, e - 127), org = (double)o.org[c];
            double lo_all = 0.0, hi_all = 0.0;
            bool have = false;
            for (int k = 0; k < 4; k++) {
                const bool empty = lo4[k] != lo4[k];
                REQUIRE(name, empty == (((o.meta >> (24 + k)) & 1u) != 0u));
                if (empty) continue;
                const double pl = org + (double)((qlo[c] >> (8 * k)) & 255u) * cell, ph = org + (double)((qhi[c] >> (8 * k)) & 255u) * cell;
                REQUIRE(name, pl <= (double)lo4[k] && ph >= (double)hi4[k]);
                lo_all = have ? std::min(lo_all, (double)lo4[k]) : (double)lo4[k];
                hi_all = have ? std::max(hi_all, (double)hi4[k]) : (double)hi4[k];
                have = true;
            }
            REQUIRE(name, have && org == lo_all);
            REQUIRE(name, e >= 60 && std::ceil((hi_all - lo_all) / cell) <= 255.0);
            REQUIRE(name, e == 60 || std::ceil((hi_all - lo_all) / std::ldexp(1.0, e - 1 - 127)) > 255.0);
            if (hi_all == lo_all) REQUIRE(name, e == 60);
        }
    }
}

void check_leaf_boxes_and_pairs(const std::string& name, const rspt_scene_desc& d) {
    const std::vector<float4> lb = leaf_boxes(&d);
    REQUIRE(name, lb.size() == 2 * d.n_prims);
    std::vector<uint32_t> pair_of(d.n_nodes, RSPT_NONE);
    uint32_t n_interior = 0;
    for (uint64_t i = 0; i < d.n_nodes; i++) {
        const rspt_bvh_node& n = d.nodes[i];
        if (n.n_prims == 0) { pair_of[i] = n_interior++; continue; }
        const float4 a = lb[2 * (size_t)n.offset], b = lb[2 * (size_t)n.offset + 1];
        REQUIRE(name, same_bits(a.x, n.bmin[0]) && same_bits(a.y, n.bmin[1]) && same_bits(a.z, n.bmin[2]) && same_bits(a.w, n.bmax[0]) && same_bits(b.x, n.bmax[1]) && same_bits(b.y, n.bmax[2]));
    }
    if (d.n_nodes < 2) return;
    const std::vector<PairNode> pairs = build_pairs(&d);
    REQUIRE(name, pairs.size() == n_interior);
    for (uint64_t i = 0; i < d.n_nodes; i++) {
        const rspt_bvh_node& n = d.nodes[i];
        if (n.n_prims) continue;
        const PairNode& p = pairs[pair_of[i]];
        const uint32_t ci[2] = {(uint32_t)i + 1u, (uint32_t)n.offset};
        const rspt_bvh_node& a = d.nodes[ci[0]], &b = d.nodes[ci[1]];
        REQUIRE(name, p.self == (uint32_t)i && p.axis == n.axis);
        REQUIRE(name, p.c0 == (a.n_prims ? (ci[0] | RSPT_REF_LEAF) : pair_of[ci[0]]) && p.c1 == (b.n_prims ? (ci[1] | RSPT_REF_LEAF) : pair_of[ci[1]]));
        const float4 q[3] = {p.q0, p.q1, p.q2};
        for (int c = 0; c < 3; c++) REQUIRE(name, same_bits(q[c].x, a.bmin[c]) && same_bits(q[c].y, b.bmin[c]) && same_bits(q[c].z, a.bmax[c]) && same_bits(q[c].w, b.bmax[c]));
    }
}

// every invariant of one scene's records; returns them
W4Records check_records(const std::string& name, const Scene& s) {
    const rspt_scene_desc d = s.desc();
    SceneFacts f;
    SceneMaterials m;
    const Error e = prepare_scene(&d, &f, &m);
    if (e) die(name, "refused: " + e.text);
    const W4Records w = build_w4(&d, f);
    Walk walk{name, &d, &f, &w, std::vector<uint32_t>(d.n_prims, 0u)};
    REQUIRE(name, w.w4_ok && w.obj_root.size() == d.n_objects && w.inst_cont.size() == d.n_instances);
    // the top level: every one of its primitives once; its records come first, a breadth-first prefix of them in front
    walk.tree(w.w4_root, 0u);
    REQUIRE(name, w.w4_top == std::min<size_t>(walk.n_records, RSPT_W4_TOP_MAX) && (f.instanced || walk.n_records == w.recs.size()));
    for (uint64_t i = 0; i < d.n_prims; i++) REQUIRE(name, walk.seen[i] == (i < f.n_top_prims ? 1u : 0u));
    // every object: exactly its own range
    for (uint32_t o = 0; o < d.n_objects; o++) {
        const rspt_object& ob = d.objects[o];
        std::fill(walk.seen.begin(), walk.seen.end(), 0u);
        if (ob.n_nodes == 0) { const auto r = walk.range(w.obj_root[o]); REQUIRE(name, r.first == ob.first_prim && r.second == 1u); walk.seen[r.first]++; }
        else walk.tree(w.obj_root[o], (uint32_t)ob.first_node);
        for (uint64_t i = 0; i < d.n_prims; i++) REQUIRE(name, walk.seen[i] == (i >= ob.first_prim && i < ob.first_prim + ob.n_prims ? 1u : 0u));
    }
    // every instance: the rest of its leaf
    std::vector<uint32_t> want(d.n_instances, RSPT_NONE);
    for (uint64_t ni = 0; ni < f.n_top_nodes && f.instanced; ni++) {
        const rspt_bvh_node& n = d.nodes[ni];
        for (uint32_t i = 0; i < n.n_prims; i++) {
            const rspt_prim& p = d.prims[(uint32_t)n.offset + i];
            if (p.mesh != RSPT_MESH_INSTANCE) continue;
            if (i + 1u == n.n_prims) { REQUIRE(name, w.inst_cont[p.v[0]] == RSPT_NONE); continue; }
            const auto r = walk.range(w.inst_cont[p.v[0]]);
            REQUIRE(name, r.first == (uint32_t)n.offset + i + 1u && r.second == n.n_prims - i - 1u);
        }
    }
    if (!w.recs.empty() && !f.instanced) check_quad4(name, w.recs);
    if (!f.instanced) check_leaf_boxes_and_pairs(name, d);
    pass("records of " + name + ": " + std::to_string(w.recs.size()) + " four-box records, " + std::to_string(w.big_leaves.size()) + " big leaves");
    return w;
}

// triangles with random vertices in a 100^3 box, sides up to 5; an aggregate from rspt_bvh_build with one primitive per leaf
Scene random_scene(uint32_t n) {
    Scene s = scene_of_triangles(0);
    s.P.clear();
    uint64_t st = 0x2545f4914f6cdd1dull;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (float)(st >> 40) / 16777216.0f; };
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < n; i++) {
        const float c[3] = {100.0f * rnd(), 100.0f * rnd(), 100.0f * rnd()};
        for (int v = 0; v < 3; v++)
            for (int k = 0; k < 3; k++) s.P.push_back(c[k] + 5.0f * rnd());
        idx.insert(idx.end(), {3 * i, 3 * i + 1, 3 * i + 2});
    }
    s.nodes.resize(2 * (size_t)n);
    std::vector<uint32_t> order(n);
    const int64_t n_nodes = rspt_bvh_build(s.P.data(), idx.data(), n, 1, s.nodes.data(), s.nodes.size(), order.data(), 1);
    if (n_nodes <= 0) die("rspt_bvh_build", rspt_bvh_last_error());
    s.nodes.resize((size_t)n_nodes);
    for (uint32_t k = 0; k < n; k++) s.prims.push_back(tri_prim(3 * order[k], 3 * order[k] + 1, 3 * order[k] + 2));
    return s;
}

void record_cases() {
    {   // a one-leaf root
        Scene s = scene_of_triangles(2);
        s.nodes = {leaf_node(0, 2, -1.0f, 1.0f)};
        const W4Records w = check_records("a one-leaf root", s);
        REQUIRE("a one-leaf root", w.recs.empty() && (w.w4_root & RSPT_REF_LEAF) && w.w4_top == 0u);
    }
    {   // root plus two leaves
        const W4Records w = check_records("a root over two leaves", base_scene());
        REQUIRE("a root over two leaves", w.recs.size() == 1 && w.w4_root == 0u && (w.recs[0].ref[0] & RSPT_REF_LEAF) && (w.recs[0].ref[2] & RSPT_REF_LEAF));
        REQUIRE("a root over two leaves", w.recs[0].ref[3] == RSPT_NONE && w.recs[0].b[0].y != w.recs[0].b[0].y && w.recs[0].b[3].y != w.recs[0].b[3].y);
    }
    for (uint32_t levels : {3u, 4u, 5u, 6u, 64u}) check_records("a chain " + std::to_string(levels) + " levels deep", chain_scene(levels));
    {   // leaves of 16 primitives go through big_leaves; 15 do not
        Scene s = scene_of_triangles(16);
        s.nodes = {leaf_node(0, 16, -1.0f, 1.0f)};
        const W4Records w = check_records("a root leaf of 16 primitives", s);
        REQUIRE("a root leaf of 16 primitives", w.big_leaves.size() == 1 && w.big_leaves[0].x == 0u && w.big_leaves[0].y == 16u);
        Scene t = scene_of_triangles(32);
        t.nodes = {interior_node(2, 2, -1.0f, 1.0f), leaf_node(0, 15, -1.0f, 0.0f), leaf_node(15, 17, 0.0f, 1.0f)};
        const W4Records v = check_records("leaves of 15 and 17 primitives", t);
        REQUIRE("leaves of 15 and 17 primitives", v.big_leaves.size() == 1 && v.big_leaves[0].x == 15u && v.big_leaves[0].y == 17u);
    }
    {   // flat boxes: the cell exponent stays at its floor
        Scene s = base_scene();
        for (rspt_bvh_node& n : s.nodes) n.bmin[2] = n.bmax[2] = 0.0f;
        const W4Records w = check_records("a flat scene", s);
        std::vector<Quad4Node> q;
        REQUIRE("a flat scene", quantise_w4(w.recs, &q) && ((q[0].meta >> 16) & 255u) == 60u);
        std::vector<Wide4Node> bad = w.recs;
        bad[0].b[1].z = Inf;
        REQUIRE("a non-finite box", !quantise_w4(bad, &q));
        bad = w.recs; bad[0].b[0].x = -3.0e38f; bad[0].b[0].z = 3.0e38f;   // an extent no 2^60 cell covers in 255 steps
        REQUIRE("a box beyond the grid", !quantise_w4(bad, &q));
        pass("quantise_w4 refuses a non-finite box and one beyond the grid");
    }
    {   // more records than the breadth-first prefix holds: the smallest such count of random triangles
        uint32_t n = RSPT_W4_TOP_MAX + 2;
        auto n_recs = [](uint32_t k) { const Scene s = random_scene(k); const rspt_scene_desc d = s.desc(); SceneFacts f; f.n_top_prims = k; f.n_top_nodes = d.n_nodes; return build_w4(&d, f).recs.size(); };
        while (n_recs(n) <= RSPT_W4_TOP_MAX) n += 16;
        while (n_recs(n - 1) > RSPT_W4_TOP_MAX) n--;
        const W4Records w = check_records(std::to_string(n) + " random triangles (the smallest count past " + std::to_string(RSPT_W4_TOP_MAX) + " records)", random_scene(n));
        REQUIRE("random triangles", w.recs.size() > RSPT_W4_TOP_MAX && w.w4_top == RSPT_W4_TOP_MAX);
        check_records("3000 random triangles", random_scene(3000));
    }
    {   // two objects, three instances, one instance in the middle of a top-level leaf
        const Scene s = instanced_scene();
        const W4Records w = check_records("two objects, three instances", s);
        REQUIRE("instances", w.recs.size() == 1 && (w.w4_root & RSPT_REF_LEAF) && w.obj_root[0] == 0u && (w.obj_root[1] & RSPT_REF_LEAF));
        REQUIRE("instances", w.inst_cont[0] != RSPT_NONE && w.inst_cont[1] != RSPT_NONE && w.inst_cont[2] == RSPT_NONE);
        const rspt_scene_desc d = s.desc();
        std::vector<InstDev> ins;
        std::vector<InstAnim> anims;
        build_instances(&d, w.obj_root, &ins, &anims);
        REQUIRE("instances", ins.size() == 3 && anims.empty() && ins[0].w4_root == 0u && ins[0].root_node == 1u && ins[0].first_prim == 4u && ins[2].root_node == RSPT_MISS && ins[2].first_prim == 6u);
        REQUIRE("instances", ins[1].identity == 0u && ins[1].anim == RSPT_MISS && ins[1].m[3] == 2.0f && ins[1].mi[3] == -2.0f && ins[1].m3[3] == 1.0f);
        pass("instance records name their object's aggregate");
    }
}

void table_cases() {
    uint32_t off[16] = {0};
    REQUIRE("pyramid_offsets", pyramid_offsets(4, 2, 3, off) == 11 && off[0] == 0 && off[1] == 8 && off[2] == 10);
    REQUIRE("pyramid_offsets", pyramid_offsets(2, 8, 4, off) == 16 + 4 + 2 + 1 && off[1] == 16 && off[2] == 20 && off[3] == 22);
    pass("pyramid_offsets of 4x2 and 2x8");
    // Distribution1D::new, restated: the running sum of f / n, normalised by its last value, or k / n when that is zero
    auto restated = [](const float* f, uint32_t n, std::vector<float>* cdf) {
        cdf->assign(n + 1, 0.0f);
        for (uint32_t k = 0; k < n; k++) (*cdf)[k + 1] = (*cdf)[k] + f[k] / (float)n;
        const float total = (*cdf)[n];
        for (uint32_t k = 1; k <= n; k++) (*cdf)[k] = total == 0.0f ? (float)k / (float)n : (*cdf)[k] / total;
        return total;
    };
    const rspt_envmap e = envmap_4x2();
    const EnvDist dist = build_env_dist(e);
    REQUIRE("envmap distribution", dist.cdf.size() == 10 && dist.fint.size() == 2 && dist.mcdf.size() == 3);
    std::vector<float> c;
    for (uint32_t v = 0; v < 2; v++) {
        const float fi = restated(DIST_4x2 + 4 * v, 4, &c);
        REQUIRE("envmap distribution", same_bits(fi, dist.fint[v]));
        for (uint32_t k = 0; k <= 4; k++) REQUIRE("envmap distribution", same_bits(c[k], dist.cdf[5 * v + k]));
    }
    REQUIRE("envmap distribution", dist.fint[1] == 0.0f && dist.cdf[6] == 0.25f && dist.cdf[9] == 1.0f);   // the all-zero row: uniform
    const float mi = restated(dist.fint.data(), 2, &c);
    REQUIRE("envmap distribution", same_bits(mi, dist.marg_int) && same_bits(c[1], dist.mcdf[1]) && dist.mcdf[0] == 0.0f && dist.mcdf[2] == 1.0f);
    pass("dist1d and the envmap distribution of a 4x2 map with an all-zero row");
    float lut[RSPT_EWA_LUT];
    ewa_weights(lut);
    REQUIRE("ewa", same_bits(lut[0], 1.0f - std::exp(-2.0f)) && lut[RSPT_EWA_LUT - 1] == 0.0f);
    pass("EWA weights run from 1 - e^-2 to 0");
    {   // the image pool and the in-line alpha masks
        Scene s = base_scene();
        s.UV = {0, 0, 1, 0, 1, 1, 0, 1};
        s.imgs = {image_4x2(), image_4x2()};
        s.texs.push_back(image_tex(1));
        s.meshes.push_back(s.meshes[0]); s.meshes[1].alpha_tex = 3; s.meshes[1].shadow_alpha_tex = 1; s.meshes[1].has_uv = 1; s.prims[1].mesh = 1;
        const rspt_scene_desc d = s.desc();
        std::vector<ImageDev> imgs;
        std::vector<float> pool;
        std::vector<uint64_t> base;
        build_image_pool(&d, &imgs, &pool, &base);
        REQUIRE("image pool", pool.size() == 66 && base.size() == 2 && base[1] == 33 && imgs[1].texel_base == 33 && imgs[1].level_offset[2] == 10 && !memcmp(pool.data() + 33, TEXELS_4x2, sizeof TEXELS_4x2));
        AlphaMasks am = build_alpha_masks(&d, base, true);
        REQUIRE("alpha masks", am.simple && am.entries.size() == 1 && am.mesh_mask[1] == 0u && am.entries[0].alpha.kind == 2u && am.entries[0].alpha.base == 33 && am.entries[0].shadow.kind == 1u && am.entries[0].shadow.value == 0.5f);
        REQUIRE("alpha masks", !build_alpha_masks(&d, base, false).simple && !build_alpha_masks(&d, std::vector<uint64_t>(), true).simple);
        pass("the image pool and the in-line alpha masks");
    }
    {   // disks and cylinders take the sphere slots behind the spheres
        Scene s = shape_scene(RSPT_MESH_CYLINDER);
        s.prims[0] = rspt_prim{{0, 0, 0}, RSPT_MESH_DISK, 0u, -1};
        s.lights.clear();
        const rspt_scene_desc d = s.desc();
        const std::vector<rspt_prim> pv = quadric_prims_as_sphere_slots(&d);
        REQUIRE("quadric slots", pv[0].mesh == RSPT_MESH_SPHERE && pv[0].v[0] == 1u && pv[1].mesh == RSPT_MESH_SPHERE && pv[1].v[0] == 2u);
        const std::vector<QuadricDev> q = quadric_slots(&d);
        REQUIRE("quadric slots", q.size() == 3 && q[0].kind == QK_SPHERE && q[1].kind == QK_DISK && q[2].kind == QK_CYLINDER && q[2].c.z_min == -1.0f);
        pass("disk and cylinder primitives name the slots behind the spheres");
    }
}

}  // namespace

int main() {
    refusal_cases();
    record_cases();
    table_cases();
    printf("%d cases passed\n", n_cases);
    return 0;
}
