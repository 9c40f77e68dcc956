// librspt.so — host side of the C ABI in include/rspt.h: scene upload, wavefront scheduling of
// the gfx950 kernels (kernels.h), film read-back.  gfx950 only; there is no CPU fallback: every
// entry point that needs the GPU fails with RSPT_E_NODEVICE / RSPT_E_HIP when it is not there.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rspt.h"
#include "material_assembly.h"
#include "scene_materials.h"
#include "scene_records.h"
#include "camera_anim.h"
#include "motion_bounds.h"
#include "kernels.h"
#include "trace_w4.h"
#include "trace_w4q.h"
#include "bvh_device.h"
#include "direct.h"
#include "vol.h"
#include "tile_serial.h"
#include "lane_serial.h"
// the heavy kernel templates are compiled in tu_*.hip; here they are only declared (tu_decl.h)
#define RSPT_TU_X extern
#define RSPT_TU_ALL
#include "tu_decl.h"

using namespace rspt;

namespace {

thread_local std::string g_err;
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return fail(RSPT_E_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
    } while (0)

struct Ctx {
    bool inited = false;
    int device = 0;
    int n_cus = 256;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // shadow-ray trace launches run beside the closest-hit launches (RSPT_TRACE_STREAMS)
    // path state
    size_t cap = 0;
    PathBuf pb{};
    // round 6, MOVING path state (kernels.h PathBuf::move): the second set of the fields a path carries from position to position (iteration it reads set it & 1: set 0 =
    // pb's own arrays, set 1 = these), the original-slot words of both sets, and the radiance of ended paths by original slot
    struct MoveSet { rspt_ray* ray_cont = nullptr; float4* L_eta = nullptr; float4* beta = nullptr; float4* nee_c1 = nullptr; uint64_t* sobol_index = nullptr;
                     uint32_t* state = nullptr; uint32_t* orig[2] = {nullptr, nullptr}; float4* L_final = nullptr /* the second carried-radiance array (move_pathbuf) */; size_t cap = 0; } mv;
    uint32_t* q[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};  // [parity][active, closest, any]
    QueueCounts* cnt = nullptr;
    uint32_t n_cnt = 0;
    uint32_t* ovf = nullptr;           // queue entries of rays whose traversal stack overflowed (k_trace_fixup's work list)
    size_t ovf_cap = 0;
    uint2* spill = nullptr;            // k_trace_w4's stack rows beyond its LDS column (trace_w4.h)
    size_t spill_threads = 0;
    VolBuf vol{};                      // volpath: per-path medium / shadow-ray state (vol.h)
    size_t vol_cap = 0;
    CamAnim* cam_anim = nullptr;       // a moving camera's key decompositions (dev_scene.h), written per render
    DlBuf dl{};                        // directlighting: per-node arrays (direct.h) + level queues
    uint32_t* dl_queue = nullptr;
    size_t dl_cap = 0;
    uint8_t* bin_keys = nullptr;       // K7b: class of every active-queue entry, the queue sorted by class, per-iteration bin bookkeeping
    uint32_t* q_sorted = nullptr;
    size_t bin_cap = 0;
    BinInfo* bin_info = nullptr;
    uint32_t n_bin_info = 0;
    uint32_t* hit_inst = nullptr;      // per path slot: instance of the continuation ray's hit (scenes with object instances)
    size_t hit_inst_cap = 0;
    float* path_time = nullptr;        // per path slot: Ray.time (scenes with moving instances)
    size_t time_cap = 0;
    float* ray_weight = nullptr;       // per path slot: the realistic camera's ray weight (kernels.h PathBuf::ray_weight)
    size_t ray_weight_cap = 0;
    float4* cam_diff = nullptr;        // per path slot: the realistic camera's differentials for the texture stage (PathBuf::cam_diff), 3 per slot
    size_t cam_diff_cap = 0;
    rspt_lens_element* lens_elements = nullptr;   // the realistic camera's two tables, uploaded per render (render_run.h upload_lens)
    float* lens_bounds = nullptr;
    unsigned long long* totals = nullptr;  // [0] nodes [1] tris [2] bsdf hits [3] rays closest [4] rays any [5] nan samples
    // sampler tables + filter table
    uint32_t* sobol32 = nullptr;
    uint64_t* vdc = nullptr;
    uint64_t* vdc_inv = nullptr;
    float* filter_table = nullptr;
    uint32_t* primes = nullptr;        // Halton: PRIMES, PRIME_SUMS, RADICAL_INVERSE_PERMUTATIONS prefix
    uint32_t* prime_sums = nullptr;
    uint16_t* halton_perms = nullptr;
    uint64_t n_halton_perms = 0;
    std::vector<uint32_t> host_primes, host_prime_sums;
    // film
    float4* film_own = nullptr;
    float4* film_splat = nullptr;
    float4* film_out = nullptr;
    size_t film_px = 0;
    uint32_t* pix_list = nullptr;
    size_t pix_cap = 0;
    uint32_t* pix_index = nullptr;     // k_film_gather: pixel of the sample-bounds grid -> its position in the pixel list
    size_t pix_index_cap = 0;
    std::vector<hipEvent_t> events;
    uint32_t tex_rows = 0;             // rows of g.pb.tex per path: RSPT_TEX_ROWS, + RSPT_DYN_ROWS once a scene with dynamic materials was rendered
    QueueCounts* look = nullptr;       // pinned host words the render loops read queue lengths into: a device-to-host copy into pageable memory
                                       // goes through a staging buffer and costs milliseconds per look (volpath looks once per pass)
};
Ctx g;

// X1: the one collective of the multi-GPU decomposition, ncclReduce(sum) of the per-rank films onto rank 0
// over xGMI.  RCCL is bound at run time so that single-GPU hosts need no librccl; a process that already has one loaded
// (torch ships its own copy) shares it.
// Before that reduce the ranks agree on whether every one of them got that far (ncclAllReduce(max) of one status word): a rank whose
// render failed contributes 1 from rspt_render's exit path, and all ranks return (RSPT_E_PEER for the healthy ones) instead of
// waiting in a collective that one member never enters.
// The handful of RCCL types the dlopen'ed entry points take, declared here with rccl.h's values (ncclInt32 = 2, ncclFloat32 = 7,
// ncclSum = 0, ncclMax = 2, NCCL_UNIQUE_ID_BYTES = 128) so that a host without the RCCL development headers still builds the library.
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt32 = 2, ncclFloat32 = 7 } ncclDataType_t;
typedef enum { ncclSum = 0, ncclMax = 2 } ncclRedOp_t;
struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 0;
    int32_t* status = nullptr;      // device word of the status agreement
    int32_t* status_host = nullptr; // its pinned host twin
    bool status_exchanged = false;  // this rspt_render call has taken part in the agreement
};
Rccl rc_;

int rccl_bind() {
    if (rc_.handle) return RSPT_OK;
    const char* names[] = {getenv("RSPT_RCCL_LIB"), "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    // one policy for every caller (rspt_comm_library): a librccl the process has mapped ALREADY wins — a second copy of RCCL in one process
    // means two sets of bootstrap threads and IPC state.  /proc/self/maps names it whatever name it was loaded by (torch ships its own copy).
    if (FILE* maps = fopen("/proc/self/maps", "r")) {
        char line[4096];
        while (!h && fgets(line, sizeof line, maps)) {
            char* path = strchr(line, '/');
            if (!path || !strstr(path, "librccl.so")) continue;
            path[strcspn(path, "\n")] = 0;
            h = dlopen(path, RTLD_NOW | RTLD_NOLOAD);
        }
        fclose(maps);
    }
    for (const char* n : names)
        if (!h && n && *n && (h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
    for (size_t i = 0; !h && i < sizeof names / sizeof *names; i++)
        if (names[i] && *names[i]) h = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(RSPT_E_UNSUPPORTED, "librccl.so not found (%s); set RSPT_RCCL_LIB", dlerror());
    *(void**)&rc_.GetUniqueId = dlsym(h, "ncclGetUniqueId");
    *(void**)&rc_.CommInitRank = dlsym(h, "ncclCommInitRank");
    *(void**)&rc_.Reduce = dlsym(h, "ncclReduce");
    *(void**)&rc_.AllReduce = dlsym(h, "ncclAllReduce");
    *(void**)&rc_.CommDestroy = dlsym(h, "ncclCommDestroy");
    *(void**)&rc_.GetErrorString = dlsym(h, "ncclGetErrorString");
    if (!rc_.GetUniqueId || !rc_.CommInitRank || !rc_.Reduce || !rc_.AllReduce || !rc_.CommDestroy || !rc_.GetErrorString)
        return fail(RSPT_E_UNSUPPORTED, "librccl.so lacks an nccl* entry point");
    rc_.handle = h;
    return RSPT_OK;
}
#define RCCL_TRY(expr)                                                                                              \
    do {                                                                                                           \
        ncclResult_t r_ = (expr);                                                                                  \
        if (r_ != ncclSuccess) return fail(RSPT_E_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, rc_.GetErrorString(r_)); \
    } while (0)

// The status agreement in front of the film reduce: every rank contributes 0 (ready to reduce) or 1 (failed); returns the maximum.
// The device word and its pinned host twin are allocated by rspt_comm_init, so that a rank that reports a failure allocates nothing on the
// way.  What the agreement covers: every failure that leaves the device usable (argument validation, UNSUPPORTED, out of memory).  After a
// sticky HIP error (a kernel fault) the copies below fail too and this rank cannot enter the collective: its peers are then released by the
// communicator's own time-out / abort, not by this word.
int film_reduce_agree(int32_t mine, int32_t* all) {
    if (!rc_.status) HIP_TRY(hipMalloc((void**)&rc_.status, sizeof(int32_t)));
    if (!rc_.status_host) HIP_TRY(hipHostMalloc((void**)&rc_.status_host, sizeof(int32_t), hipHostMallocDefault));
    *rc_.status_host = mine;
    HIP_TRY(hipMemcpyAsync(rc_.status, rc_.status_host, sizeof mine, hipMemcpyHostToDevice, g.stream));
    rc_.status_exchanged = true;
    RCCL_TRY(rc_.AllReduce(rc_.status, rc_.status, 1, ncclInt32, ncclMax, rc_.comm, g.stream));
    HIP_TRY(hipMemcpyAsync(rc_.status_host, rc_.status, sizeof *all, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    *all = *rc_.status_host;
    return RSPT_OK;
}

struct LightDist {
    float* func = nullptr;
    float* cdf = nullptr;
    float* func_int = nullptr;
    int32_t nvox[3] = {1, 1, 1};
    int32_t spatial = 0;
    // on-demand voxels: table (one int32 per voxel), the list of voxels claimed in the current round, the counters
    int32_t* table = nullptr;
    uint32_t* new_list = nullptr;
    LightLazy* lazy = nullptr;
    uint32_t max_rows = 0;
};

}  // namespace

struct rspt_scene_s {
    SceneDev dev{};
    const PairNode* pairs = nullptr;  // one per interior LinearBVHNode (trace_wide.h)
    const Wide4Node* w4 = nullptr;    // one per interior LinearBVHNode at even depth (trace_w4.h)
    const uint2* big_leaves = nullptr;
    uint32_t w4_root = 0;
    uint32_t w4_top = 0;              // records kept in LDS by k_trace_w4 (a breadth-first prefix, numbered first)
    bool w4_ok = false;               // false: too large for the ref fields, k_trace_pw serves the scene
    const Quad4Node* w4q = nullptr;   // the same records on an 8-bit grid, for the shadow-ray kernel k_trace_w4q (trace_w4q.h): plain scenes only (no instances, no alpha masks)
    const float4* leaf_boxes = nullptr;  // [2 * first primitive of a leaf]: the leaf's LinearBVHNode bounds, for that kernel's exact leaf test
    int camera_pk_choice = -1;        // which kernel serves this scene's camera-ray launches: -1 not measured yet (k_trace_w4 until then), 0 k_trace_w4, 1 k_trace_w4pk (trace_packet.h), 2 k_trace_w4pf (trace_frustum.h), 3 / 4 k_trace_w4pb with bundles of two / four packets (trace_bundle.h) —
                                      // set by the first large camera launch of a path render, which runs all five on the same rays and keeps the fastest (RenderRun::tune_camera)
    int any_q_choice = -1;            // which kernel serves this scene's shadow rays: -1 not measured yet (the plain one until then), 0 k_trace_w4<true>, 1 k_trace_w4q — set by
                                      // the first large shadow-ray launch of a render, which runs both on the same rays and keeps the faster (RenderRun::tune_any)
    TexTables tex{};                  // textures / images / per-material slots (dev_texture.h); has_textures says whether set
    bool has_textures = false;
    // Lobe lists as material_assembly.h built them, once per value of the integrator's allow_multiple_lobes ([0]: true — path,
    // volpath, ao; [1]: false — directlighting: glass as SpecularReflection + SpecularTransmission, glass.rs:136-188).
    // select_materials() points dev / tex at the set a render needs.
    struct MatSet {
        const rspt_material* materials = nullptr;
        const rspt_bxdf* bxdfs = nullptr;
        const uint32_t* mat_slots = nullptr;
        const uint8_t* mat_flags = nullptr;
        const rspt_mat::DynMaterial* dyn = nullptr;
        bool textured = false, dynamic = false;
    } mat_set[2];
    bool has_dynamic = false;         // (in the selected set) some material's lobe list is built per hit
    uint32_t shade_features = 0;      // SF_* (dev_bsdf.h) of everything the scene can put in front of the shade stage
    uint32_t shade_classes = 1;       // distinct lobe-list shapes among the materials: K7b sorts the shade queue by material only when waves would differ
    void select_materials(bool allow_multiple_lobes) {
        const MatSet& m = mat_set[allow_multiple_lobes ? 0 : 1];
        dev.materials = m.materials; dev.bxdfs = m.bxdfs;
        tex.mat_slots = m.mat_slots; tex.mat_flags = m.mat_flags;
        dev.mat_flags = m.textured ? m.mat_flags : nullptr;
        dev.dyn = m.dyn; tex.dyn = m.dyn;
        has_textures = m.textured;
        has_dynamic = m.dynamic;
    }
    std::vector<void*> allocs;        // every device allocation of the scene: freed with it
    rspt_scene_s() = default;
    rspt_scene_s(const rspt_scene_s&) = delete;
    rspt_scene_s& operator=(const rspt_scene_s&) = delete;
    ~rspt_scene_s() { for (void* p : allocs) (void)hipFree(p); }
    bool has_null_material = false;
    uint32_t n_materials = 0;
    bool has_alpha = false;           // some mesh carries an alpha / shadow-alpha mask (Triangle::intersect's alpha tests)
    bool alpha_simple = false;        // ... and every mask is a constant or a uv-mapped image (dev_scene.h AlphaMask): k_trace_w4<.., ALPHA = 2>
    std::vector<uint64_t> image_base; // per image: its first float in the texel pool
    bool has_instances = false;       // object instances: two-level traversal (kernels.h traverse<ANY, true>)
    bool has_animated = false;        // ... some of them moving (dev_scene.h inst_at): the reference-order kernel serves the scene, `path` under Sobol' / Halton only
    const char* maplight_kinds = "";   // "projection", "goniometric" or "projection and goniometric": which of the two the scene holds, for the refusals
    bool has_maplights = false;       // ABI 24: a projection or goniometric light (dev_scene.h light_sample_li's two arms); rspt_render serves them under path (Sobol', Halton) and ao
    bool has_spheres = false;         // ABI 23: analytic spheres behind the triangle records (dev_sphere.h); rspt_render serves them under path / ao (Sobol', Halton)
    bool has_sphere_light = false;    // an emissive sphere: refused by rspt_render and the light-distribution hook unless the sphere-light gate is on (rspt_set_sphere_lights)
    // ABI 27: a disk or a cylinder (dev_quadric.h).  Such a scene also sets has_spheres — its records sit in the sphere slots and it takes every path a sphere scene
    // takes — and has_quadrics picks the instantiations that read a slot's kind.  quadric_kinds / quadric_light_kinds: "disk", "cylinder" or "disk and cylinder", for the refusals
    bool has_quadrics = false, has_disks = false, has_cylinders = false;
    const char* quadric_kinds = "";
    const char* quadric_light_kinds = nullptr, *quadric_light_what = "";   // which of them emit ("disk", .. / "disk area lights", ..): refused by rspt_render and the light-distribution hook (Disk::sample / Cylinder::sample are not on the device)
    std::map<int, LightDist> light_dists;  // by effective strategy
};

namespace {

template <class T>
int dev_alloc(T** out, size_t n) {
    *out = nullptr;
    if (n == 0) return RSPT_OK;
    HIP_TRY(hipMalloc((void**)out, n * sizeof(T)));
    return RSPT_OK;
}
// a device array that only grows: free, null, zero the capacity, allocate, set the capacity
template <class T, class N>
int ensure_array(T** p, N* cap, size_t n) {
    if (*cap >= n) return RSPT_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    int rc = dev_alloc(p, n);
    if (rc) return rc;
    *cap = (N)n;
    return RSPT_OK;
}
template <class T>
int upload(rspt_scene_s* s, const T* host, size_t n, const T** out) {
    *out = nullptr;
    if (n == 0 || !host) return RSPT_OK;
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, n * sizeof(T)));
    s->allocs.push_back(d);
    HIP_TRY(hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)d;
    return RSPT_OK;
}

uint32_t grid_for(uint32_t waves_per_cu_blocks) { return (uint32_t)g.n_cus * waves_per_cu_blocks; }

size_t env_size(const char* name, size_t dflt) {
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    return (size_t)strtoull(v, nullptr, 0);
}

void free_move() {
    void* ptrs[] = {g.mv.ray_cont, g.mv.L_eta, g.mv.beta, g.mv.nee_c1, g.mv.sobol_index, g.mv.state, g.mv.orig[0], g.mv.orig[1], g.mv.L_final};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    g.mv = Ctx::MoveSet{};
}
void free_paths() {
    free_move();
    void* ptrs[] = {g.pb.ray_cont, g.pb.ray_mis, g.pb.ray_sh, g.pb.hit_cont, g.pb.hit_mis, g.pb.occluded, g.pb.L_eta, g.pb.beta,
                    g.pb.nee_c1, g.pb.nee_c2, g.pb.nee_beta, g.pb.sobol_index, g.pb.state, g.pb.p_film, g.pb.tex, g.pb.dyn_built,
                    g.q[0][0], g.q[0][1], g.q[0][2], g.q[1][0], g.q[1][1], g.q[1][2]};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (g.path_time) (void)hipFree(g.path_time);   // sized with the path buffers (RenderRun::prepare), freed with them
    g.path_time = nullptr; g.time_cap = 0;
    if (g.ray_weight) (void)hipFree(g.ray_weight);   // the realistic camera's per-slot arrays: sized and freed the same way
    if (g.cam_diff) (void)hipFree(g.cam_diff);
    g.ray_weight = nullptr; g.ray_weight_cap = 0; g.cam_diff = nullptr; g.cam_diff_cap = 0;
    g.pb = PathBuf{};
    g.tex_rows = 0;
    for (auto& a : g.q) a[0] = a[1] = a[2] = nullptr;
    g.cap = 0;
}

int ensure_paths(size_t cap) {
    if (g.cap >= cap) return RSPT_OK;
    free_paths();
    int rc;
#define A(field, n) if ((rc = dev_alloc(&field, (n))) != RSPT_OK) return rc
    A(g.pb.ray_cont, cap); A(g.pb.ray_mis, cap); A(g.pb.ray_sh, cap);
    A(g.pb.hit_cont, cap); A(g.pb.hit_mis, cap); A(g.pb.occluded, cap);
    A(g.pb.L_eta, cap); A(g.pb.beta, cap); A(g.pb.nee_c1, cap); A(g.pb.nee_c2, cap); A(g.pb.nee_beta, cap);
    A(g.pb.sobol_index, cap); A(g.pb.state, cap); A(g.pb.p_film, cap);
    for (int par = 0; par < 2; par++) {
        A(g.q[par][0], cap);
        A(g.q[par][1], 2 * cap);  // continuation + MIS rays
        A(g.q[par][2], cap);
    }
#undef A
    g.cap = cap;
    return RSPT_OK;
}

// the second set of the MOVE schedule (116 B per path on top of ensure_paths' 280), sized like the first
int ensure_move(size_t cap) {
    if (g.mv.cap >= cap) return RSPT_OK;
    free_move();
    int rc;
    if ((rc = dev_alloc(&g.mv.ray_cont, cap)) || (rc = dev_alloc(&g.mv.L_eta, cap)) || (rc = dev_alloc(&g.mv.beta, cap)) || (rc = dev_alloc(&g.mv.nee_c1, cap)) ||
        (rc = dev_alloc(&g.mv.sobol_index, cap)) || (rc = dev_alloc(&g.mv.state, cap)) || (rc = dev_alloc(&g.mv.orig[0], cap)) || (rc = dev_alloc(&g.mv.orig[1], cap)) ||
        (rc = dev_alloc(&g.mv.L_final, cap)))
        return rc;
    g.mv.cap = cap;
    return RSPT_OK;
}
// the PathBuf of wavefront iteration `it` under the MOVE schedule, which starts at iteration `first` (RSPT_MOVE_FROM: the iterations before it run the slot-for-life
// kernel on set 0 = pb's own arrays): iteration it >= first reads set (it - first) & 1 and writes the other; at it == first the queue still holds original slots.
// The radiance is the exception: pb.L_eta — by original slot — is what k_film reads (L_final), so the carried radiance alternates between the two arrays of the
// second set and only the first MOVE launch reads it from pb.L_eta, where the slot-for-life launches (or nothing: a fresh batch) left it.
PathBuf move_pathbuf(uint32_t it, uint32_t first) {
    PathBuf b = g.pb;
    const Ctx::MoveSet& m = g.mv;
    b.L_final = g.pb.L_eta;
    if (it < first) return b;
    b.move = 1u;
    b.orig_is_p = it == first ? 1u : 0u;
    it -= first;
    rspt_ray* rc[2] = {g.pb.ray_cont, m.ray_cont}; float4* be[2] = {g.pb.beta, m.beta}; float4* c1[2] = {g.pb.nee_c1, m.nee_c1};
    uint64_t* so[2] = {g.pb.sobol_index, m.sobol_index}; uint32_t* st[2] = {g.pb.state, m.state}; float4* le[2] = {m.L_eta, m.L_final};
    const int r = (int)(it & 1u), w = r ^ 1;
    b.ray_cont = rc[r]; b.beta = be[r]; b.nee_c1 = c1[r]; b.sobol_index = so[r]; b.state = st[r]; b.orig = m.orig[r];
    b.L_eta = it == 0 ? g.pb.L_eta : le[w];   // (written by iteration it - 1 into le[(it - 1) & 1] = le[w])
    b.o_ray_cont = rc[w]; b.o_L_eta = le[r]; b.o_beta = be[w]; b.o_nee_c1 = c1[w]; b.o_sobol_index = so[w]; b.o_state = st[w]; b.o_orig = m.orig[w];
    return b;
}

// per-path rows of k_texture's results, only for scenes with textures (6 x 16 B per path)
int ensure_tex_rows(bool dynamic) {
    const uint32_t rows = RSPT_TEX_ROWS + (dynamic ? RSPT_DYN_ROWS : 0);
    if (g.pb.tex && g.tex_rows >= rows) return RSPT_OK;
    if (g.pb.tex) (void)hipFree(g.pb.tex);
    g.pb.tex = nullptr; g.tex_rows = 0;
    int rc = dev_alloc(&g.pb.tex, g.cap * rows);
    if (rc) return rc;
    g.pb.tex_stride = (uint32_t)g.cap;
    g.tex_rows = rows;
    return RSPT_OK;
}
// dynamic materials: one Built record (8 lobes) per thread of the widest shade-stage launch
int ensure_dyn_built(uint32_t threads) {
    return ensure_array(&g.pb.dyn_built, &g.pb.dyn_threads, threads);
}

int ensure_direct(size_t cap) {
    if (g.dl_cap >= cap) return RSPT_OK;
    void* old[] = {g.dl.le_kind, g.dl.w_r, g.dl.w_t, g.dl.l_all, g.dl.ld_acc, g.dl.dim, g.dl.kidx, g.dl.nflags, g.dl.error, g.dl_queue};
    for (void* p : old) if (p) (void)hipFree(p);
    g.dl = DlBuf{}; g.dl_queue = nullptr; g.dl_cap = 0;
    int rc;
    if ((rc = dev_alloc(&g.dl.le_kind, cap)) || (rc = dev_alloc(&g.dl.w_r, cap)) || (rc = dev_alloc(&g.dl.w_t, cap)) || (rc = dev_alloc(&g.dl.l_all, cap)) ||
        (rc = dev_alloc(&g.dl.ld_acc, cap)) || (rc = dev_alloc(&g.dl.dim, cap)) || (rc = dev_alloc(&g.dl.kidx, cap)) || (rc = dev_alloc(&g.dl.nflags, cap)) ||
        (rc = dev_alloc(&g.dl.error, 1)) || (rc = dev_alloc(&g.dl_queue, cap)))
        return rc;
    g.dl_cap = cap;
    return RSPT_OK;
}

int ensure_vol(size_t cap) {
    if (g.vol_cap >= cap) return RSPT_OK;
    void* old[] = {g.vol.medium, g.vol.sh, g.vol.p1_p, g.vol.p1_e, g.vol.p1_n, g.vol.post, g.vol.truncated};
    for (void* p : old) if (p) (void)hipFree(p);
    g.vol = VolBuf{}; g.vol_cap = 0;
    int rc;
    if ((rc = dev_alloc(&g.vol.medium, cap)) || (rc = dev_alloc(&g.vol.sh, cap)) || (rc = dev_alloc(&g.vol.p1_p, cap)) || (rc = dev_alloc(&g.vol.p1_e, cap)) ||
        (rc = dev_alloc(&g.vol.p1_n, cap)) || (rc = dev_alloc(&g.vol.post, cap)) || (rc = dev_alloc(&g.vol.truncated, 1)))
        return rc;
    g.vol_cap = cap;
    return RSPT_OK;
}

int ensure_bins(size_t cap, uint32_t n_iters) {
    int rc;
    if (g.bin_cap < cap) {
        if (g.bin_keys) (void)hipFree(g.bin_keys);
        if (g.q_sorted) (void)hipFree(g.q_sorted);
        g.bin_keys = nullptr; g.q_sorted = nullptr; g.bin_cap = 0;
        if ((rc = dev_alloc(&g.bin_keys, cap)) || (rc = dev_alloc(&g.q_sorted, cap + 64 * RSPT_BIN_K))) return rc;
        g.bin_cap = cap;
    }
    return ensure_array(&g.bin_info, &g.n_bin_info, n_iters);
}


int ensure_spill(size_t threads) {
    if (g.spill_threads >= threads) return RSPT_OK;
    if (g.spill) (void)hipFree(g.spill);
    g.spill = nullptr; g.spill_threads = 0;
    int rc = dev_alloc(&g.spill, 2 * threads * RSPT_W4_SPILL);  // one set of rows per trace lane
    if (rc) return rc;
    g.spill_threads = threads;
    return RSPT_OK;
}
// persistent trace grid = what is resident: k_trace_w4 fits five 256-thread workgroups per CU (93 VGPRs, 30 KB LDS); more only
// adds workgroups that start at the tail, copy the root-side records and find the queue empty (8 -> 5: C3 +0.6 %)
uint32_t pw_grid() { return grid_for((uint32_t)env_size("RSPT_PW_BLOCKS_PER_CU", 5)); }
// threads of the widest persistent trace launch any selectable shape can make (spill rows are addressed [row][thread]): the default shape's pw_grid() x 256, or the
// 1024 threads per CU of RSPT_W4_SHAPE = 1 / 2 — whichever is larger (with RSPT_PW_BLOCKS_PER_CU < 4 the big shapes indexed past the rows sized for the default)
size_t pw_spill_threads() { return std::max<size_t>((size_t)pw_grid() * RSPT_PW_BLOCK, (size_t)grid_for(1) * 1024u); }


hipEvent_t get_event(size_t i) {
    while (g.events.size() <= i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        g.events.push_back(e);
    }
    return g.events[i];
}

__global__ void k_accum_counts(const QueueCounts* cnt, uint32_t n_iter, unsigned long long* totals) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long c = 0, a = 0;
    for (uint32_t i = 0; i < n_iter; i++) { c += cnt[i].closest; a += cnt[i].any; }
    totals[3] += c;
    totals[4] += a;
}

// blockqueue/mod.rs:100-115
uint32_t part1by1(uint32_t x) {
    x &= 0x0000ffff; x = (x ^ (x << 8)) & 0x00ff00ff; x = (x ^ (x << 4)) & 0x0f0f0f0f;
    x = (x ^ (x << 2)) & 0x33333333; return (x ^ (x << 1)) & 0x55555555;
}
uint32_t morton2(uint32_t x, uint32_t y) { return (part1by1(y) << 1) + part1by1(x); }

int round_up_pow2_32(int32_t v) {  // pbrt.rs:188-198
    v -= 1; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16;
    return v + 1;
}

// ---- the sphere-light gate (include/rspt.h rspt_set_sphere_lights): host-only, process-wide, off by default ----
std::atomic<uint32_t> g_sphere_lights{0u};
// the gate a call runs under: RSPT_SPHERE_LIGHTS = 0 | 1 when set and non-empty, else what rspt_set_sphere_lights left; -1: the variable holds something else
int sphere_lights_mode() {
    const char* e = getenv("RSPT_SPHERE_LIGHTS");
    if (!e || !*e) return (int)g_sphere_lights.load();
    if (!strcmp(e, "0")) return 0;
    if (!strcmp(e, "1")) return 1;
    return -1;
}
// ---- the quadric-light gate (include/rspt.h rspt_set_quadric_lights): the same for disk and cylinder area lights ----
std::atomic<uint32_t> g_quadric_lights{0u};
int quadric_lights_mode() {
    const char* e = getenv("RSPT_QUADRIC_LIGHTS");
    if (!e || !*e) return (int)g_quadric_lights.load();
    if (!strcmp(e, "0")) return 0;
    if (!strcmp(e, "1")) return 1;
    return -1;
}
// the area lights on quadrics that a scene with a disk or a cylinder holds, for the refusals of a call that serves them: "disk area lights", .. or, where only
// a sphere emits there, "sphere area lights"
const char* quadric_scene_lights_what(const rspt_scene_s* s) { return s->quadric_light_kinds ? s->quadric_light_what : "sphere area lights"; }

// Light distribution for (scene, strategy): create_light_sample_distribution (lightdistrib.rs:393-418)
// (a scene with a disk or a cylinder that holds an emissive quadric reaches this only while the gates its lights need are on: the _ql kernels build its tables)
// (a scene with an emissive sphere reaches this only while the sphere-light gate is on: its tables come from the kernels that carry the sphere arm)
int get_light_dist(rspt_scene_s* s, uint32_t strategy, LightDistDev* out, const LightDist** lazy_out = nullptr) {
    const uint32_t nl = s->dev.n_lights;
    *out = LightDistDev{};
    out->nvox[0] = out->nvox[1] = out->nvox[2] = 1;
    if (nl == 0) return RSPT_OK;
    int eff = (strategy == RSPT_LIGHTS_UNIFORM || nl == 1) ? RSPT_LIGHTS_UNIFORM : (strategy == RSPT_LIGHTS_POWER ? RSPT_LIGHTS_POWER : RSPT_LIGHTS_SPATIAL);
    const bool ql = s->has_quadrics && (s->quadric_light_kinds || s->has_sphere_light);   // an area light on a quadric in a scene whose slots are QuadricDev
    auto it = s->light_dists.find(eff);
    if (it == s->light_dists.end()) {
        LightDist d;
        uint64_t n_vox = 1;
        uint64_t n_rows = 1;
        bool lazy = false;
        if (eff == RSPT_LIGHTS_SPATIAL) {  // SpatialLightDistribution::new (lightdistrib.rs:127-166)
            float diag[3] = {s->dev.wb_max[0] - s->dev.wb_min[0], s->dev.wb_max[1] - s->dev.wb_min[1], s->dev.wb_max[2] - s->dev.wb_min[2]};
            int me = (diag[0] > diag[1] && diag[0] > diag[2]) ? 0 : (diag[1] > diag[2] ? 1 : 2);  // maximum_extent
            float bmax = diag[me];
            for (int i = 0; i < 3; i++) {
                float r = roundf(diag[i] / bmax * 64.0f);
                int32_t v = (r != r) ? 0 : (r >= 2147483648.0f ? 2147483647 : (r <= -2147483648.0f ? (-2147483647 - 1) : (int32_t)r));
                d.nvox[i] = std::max(1, v);
            }
            n_vox = (uint64_t)d.nvox[0] * d.nvox[1] * d.nvox[2];
            d.spatial = 1;
            // Every emissive triangle is a light, so the full table is n_vox x n_lights (64^3 voxels x 10^4 lights = 21 GB and 3 x 10^11
            // light samples before the first pixel).  The reference fills a voxel the first time a path looks it up
            // (lightdistrib.rs:297-384); above RSPT_LIGHT_TABLE_EAGER_BYTES the same is done here, with rows handed out from a pool.
            const uint64_t row_bytes = (2ull * nl + 2ull) * sizeof(float);
            lazy = n_vox * row_bytes > env_size("RSPT_LIGHT_TABLE_EAGER_BYTES", (size_t)1 << 30);
            n_rows = n_vox;
            if (lazy) n_rows = std::max<uint64_t>(1, std::min<uint64_t>(n_vox, env_size("RSPT_LIGHT_TABLE_POOL_BYTES", (size_t)16 << 30) / row_bytes));
            // (the on-demand kernels carry no projection / goniometric arm: such a scene takes the table built up front or nothing)
            if (lazy && s->has_maplights) return fail(RSPT_E_UNSUPPORTED, "scene with a %s light whose spatial light table needs on-demand voxels (more than RSPT_LIGHT_TABLE_EAGER_BYTES)", s->maplight_kinds);
            if (lazy && ql && s->quadric_light_kinds) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive %s whose spatial light table needs on-demand voxels (more than RSPT_LIGHT_TABLE_EAGER_BYTES): the on-demand kernels carry no %s", s->quadric_light_kinds, s->quadric_light_what);
            if (lazy && s->has_sphere_light) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere whose spatial light table needs on-demand voxels (more than RSPT_LIGHT_TABLE_EAGER_BYTES): the on-demand kernels carry no sphere area light");
            if (n_rows > 0x7fffffffull || n_vox > 0x7fffffffull) return fail(RSPT_E_UNSUPPORTED, "spatial light distribution: %llu voxels", (unsigned long long)n_vox);
        }
        int rc;
        // every allocation is owned by the scene as soon as it exists (a later failure must not leak the earlier ones)
        auto owned = [&](auto** p, size_t n) { int r = dev_alloc(p, n); if (!r && *p) s->allocs.push_back(*p); return r; };
        if ((rc = owned(&d.func, n_rows * nl)) || (rc = owned(&d.cdf, n_rows * (nl + 1))) || (rc = owned(&d.func_int, n_rows))) return rc;
        if (lazy) {
            if ((rc = owned(&d.table, n_vox)) || (rc = owned(&d.new_list, n_rows)) || (rc = owned(&d.lazy, 1))) return rc;
            d.max_rows = (uint32_t)n_rows;
            HIP_TRY(hipMemsetAsync(d.table, 0xff, n_vox * sizeof(int32_t), g.stream));  // -1: no distribution yet
            LightLazy lz{0u, 0u, d.max_rows, 0u};
            HIP_TRY(hipMemcpyAsync(d.lazy, &lz, sizeof lz, hipMemcpyHostToDevice, g.stream));
        } else if (eff == RSPT_LIGHTS_SPATIAL) {
            uint64_t total = n_vox * nl;
            hipLaunchKernelGGL(ql ? k_ld_contrib_ql : s->has_sphere_light ? k_ld_contrib_sl : s->has_maplights ? k_ld_contrib_ml : k_ld_contrib, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, g.stream, s->dev, d.nvox[0], d.nvox[1], d.nvox[2], d.func);
            hipLaunchKernelGGL(k_ld_build, dim3((uint32_t)((n_vox + 255) / 256)), dim3(256), 0, g.stream, (uint32_t)n_vox, nl, 0, d.func, d.cdf, d.func_int);
        } else {
            hipLaunchKernelGGL(ql ? k_ld_fixed_ql : s->has_sphere_light ? k_ld_fixed_sl : s->has_maplights ? k_ld_fixed_ml : k_ld_fixed, dim3((nl + 255) / 256), dim3(256), 0, g.stream, s->dev, eff == RSPT_LIGHTS_POWER ? 1 : 0, d.func);
            hipLaunchKernelGGL(k_ld_build, dim3(1), dim3(64), 0, g.stream, 1u, nl, 1, d.func, d.cdf, d.func_int);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g.stream));
        it = s->light_dists.emplace(eff, d).first;
    }
    const LightDist& d = it->second;
    out->func = d.func; out->cdf = d.cdf; out->func_int = d.func_int;
    out->nvox[0] = d.nvox[0]; out->nvox[1] = d.nvox[1]; out->nvox[2] = d.nvox[2];
    out->spatial = d.spatial;
    out->table = d.table;
    if (lazy_out) *lazy_out = d.table ? &d : nullptr;
    return RSPT_OK;
}

// the render entry, included here once inside this namespace: one trace launch, the state of a render with its validation and setup, the schedules over it
#include "launch_trace.h"
#include "render_run.h"
#include "render_schedules.h"
#include "render_tile_serial.h"

int render_impl(rspt_scene_s* s, const rspt_render_desc* d, float* film_host, void* film_dev, float* li_host, rspt_stats* stats) {
    RenderRun r(s, d);
    int rc;
    if ((rc = r.validate())) return rc;
    s->select_materials(r.multi_lobes);  // allow_multiple_lobes: false in DirectLightingIntegrator::li and WhittedIntegrator::li (directlighting.rs:86, whitted.rs:63)
    auto t_start = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(g.device));
    if ((rc = r.constants()) || (rc = r.shard_pixels()) || (rc = r.film_buffers(li_host)) || (rc = r.size_batches()) || (rc = r.prepare())) return rc;
    if ((rc = r.run()) || (rc = r.finish(film_host, film_dev, li_host))) return rc;
    return r.report(stats, t_start);
}

// ---- rspt_scene_create's device steps: each takes records that scene_records.h built on the host and uploads them; the scene owns what was uploaded ----
template <class T>
int upload(rspt_scene_s* s, const std::vector<T>& v, const T** out) { return upload(s, v.data(), v.size(), out); }
#define UP(...) do { if ((rc = upload(s, __VA_ARGS__))) return rc; } while (0)

// media: a grid medium's density goes to the device, its record gets the device pointer and 1 / max(density) (GridDensityMedium::new, grid.rs:44-55)
int upload_media(rspt_scene_s* s, const rspt_scene_desc* d) {
    int rc;
    std::vector<rspt_medium> media(d->media, d->media + d->n_media);
    for (rspt_medium& m : media) {
        if (m.kind != RSPT_MEDIUM_GRID) continue;
        const float inv_max = scene::grid_inv_max_density(m);
        memcpy(&m.pad, &inv_max, sizeof inv_max);
        const float* dens_d = nullptr;
        UP(m.density, (size_t)m.nx * m.ny * m.nz, &dens_d);
        m.density = dens_d;
        s->dev.n_grid_media++;
    }
    UP(media, &s->dev.media);
    s->dev.n_media = d->n_media;
    return RSPT_OK;
}

// the two lobe sets with their slot tables; the texture tables when a material is textured (k_texture / per-path texture rows) or a mesh is alpha-masked
int upload_materials(rspt_scene_s* s, const rspt_scene_desc* d, const scene::SceneMaterials& sm) {
    int rc;
    for (int v = 0; v < 2; v++) {
        rspt_scene_s::MatSet& ms = s->mat_set[v];
        ms.textured = sm.textured[v];
        ms.dynamic = !sm.dyn[v].empty();
        if (ms.dynamic) UP(sm.dyn[v], &ms.dyn);
        UP(sm.mats[v], &ms.materials); UP(sm.bxdfs[v], &ms.bxdfs); UP(sm.slots[v], &ms.mat_slots); UP(sm.mflags[v], &ms.mat_flags);
    }
    s->select_materials(true);
    if (!sm.textured[0] && !sm.textured[1] && !s->has_alpha) return RSPT_OK;
    UP(d->textures, d->n_textures, &s->tex.textures);
    std::vector<ImageDev> imgs;
    std::vector<float> pool;
    scene::build_image_pool(d, &imgs, &pool, &s->image_base);
    UP(pool, &s->tex.texel_pool);
    UP(imgs, &s->tex.images);
    float lut[RSPT_EWA_LUT];
    scene::ewa_weights(lut);
    UP(lut, (size_t)RSPT_EWA_LUT, &s->tex.ewa_lut);
    return RSPT_OK;
}

// Scene.infinite_lights and the environment maps: each map's pyramid, and its Distribution2D unless only projection / goniometric lights name it (ABI 24)
int upload_envmaps(rspt_scene_s* s, const rspt_scene_desc* d) {
    int rc;
    const std::vector<uint32_t> inf = scene::infinite_lights(d);
    s->dev.n_infinite = (uint32_t)inf.size();
    UP(inf, &s->dev.infinite_lights);
    std::vector<EnvMapDev> envs(d->n_envmaps);
    for (uint32_t i = 0; i < d->n_envmaps; i++) {
        const rspt_envmap& e = d->envmaps[i];
        EnvMapDev& m = envs[i];
        m.width = e.width; m.height = e.height; m.n_levels = e.n_levels; m.nu = e.dist_nu; m.nv = e.dist_nv;
        UP(e.texels, scene::pyramid_offsets(e.width, e.height, e.n_levels, m.level_offset) * 3, &m.texels);
        if (!e.dist_func) continue;   // the pyramid alone, the distribution pointers stay null
        const scene::EnvDist dist = scene::build_env_dist(e);
        m.marg_int = dist.marg_int;
        UP(e.dist_func, (size_t)e.dist_nu * e.dist_nv, &m.cond_func); UP(dist.cdf, &m.cond_cdf);
        UP(dist.fint, &m.cond_int); UP(dist.fint, &m.marg_func); UP(dist.mcdf, &m.marg_cdf);
    }
    UP(envs, &s->dev.envmaps);
    return RSPT_OK;
}

// the four-box records (trace_w4.h) and, for the shadow rays of plain scenes, their quantised form with the leaf boxes (trace_w4q.h)
int upload_w4(rspt_scene_s* s, const rspt_scene_desc* d, const scene::SceneFacts& f, const scene::W4Records& w4) {
    int rc;
    s->w4_root = w4.w4_root; s->w4_top = w4.w4_top; s->w4_ok = w4.w4_ok;
    if (w4.w4_ok) UP(w4.recs, &s->w4);
    UP(w4.big_leaves, &s->big_leaves);
    // not for scenes with instances or alpha masks, nor with spheres, disks or cylinders: k_trace_w4q walks triangle leaves only, and launch_trace_sph never takes it
    if (!s->w4 || f.instanced || f.any_alpha || d->n_spheres || d->n_disks || d->n_cylinders || env_size("RSPT_W4Q_BUILD", 1) == 0) return RSPT_OK;
    std::vector<Quad4Node> q;
    if (!scene::quantise_w4(w4.recs, &q)) return RSPT_OK;
    UP(q, &s->w4q);
    UP(scene::leaf_boxes(d), &s->leaf_boxes);
    return RSPT_OK;
}

// the triangle records (k_build_tris) with the sphere / disk / cylinder slots behind them, and the in-line alpha masks they name
int build_primitive_records(rspt_scene_s* s, const rspt_scene_desc* d, const scene::SceneFacts& f, const scene::W4Records& w4, const rspt_mesh* meshes_d, const float* P_d) {
    int rc;
    float4* tris = nullptr;
    // a scene with spheres keeps them behind the triangle records (dev_sphere.h SphereDev, RSPT_SPHERE_F4 float4 each); disks and cylinders take sphere slots (ABI 27)
    const uint64_t n_slots = (uint64_t)d->n_spheres + d->n_disks + d->n_cylinders;
    hipError_t e = hipMalloc((void**)&tris, (d->n_prims * 3 + n_slots * RSPT_SPHERE_F4) * sizeof(float4));
    if (e != hipSuccess) return fail(RSPT_E_NOMEM, "triangle records: %s", hipGetErrorString(e));
    s->allocs.push_back(tris);
    const uint32_t* inst_cont_d = nullptr, *mesh_mask_d = nullptr;
    UP(w4.inst_cont, &inst_cont_d);
    if (s->has_alpha && env_size("RSPT_ALPHA_SIMPLE", 1) != 0) {
        const scene::AlphaMasks am = scene::build_alpha_masks(d, s->image_base, s->dev.tri_nuv != nullptr);
        if (am.simple && !am.entries.empty()) {
            UP(am.entries, &s->dev.alpha_masks); UP(am.mesh_mask, &mesh_mask_d);
            s->alpha_simple = true;
        }
    }
    hipLaunchKernelGGL(k_build_tris, dim3((uint32_t)((d->n_prims + 255) / 256)), dim3(256), 0, g.stream, s->dev.prims, meshes_d, P_d, (uint32_t)d->n_prims, tris, inst_cont_d, mesh_mask_d);
    e = hipStreamSynchronize(g.stream);
    if (e != hipSuccess) return fail(RSPT_E_HIP, "k_build_tris: %s", hipGetErrorString(e));
    if (d->n_spheres) {   // ABI 23 (k_build_tris wrote the sphere primitives' own records)
        const std::vector<SphereDev> sph = scene::sphere_slots(d);
        e = hipMemcpy(tris + 3 * d->n_prims, sph.data(), sph.size() * sizeof(SphereDev), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(RSPT_E_HIP, "sphere records: %s", hipGetErrorString(e));
        s->has_spheres = true;
        s->shade_features |= SF_SPHERE;
        for (uint64_t i = 0; i < d->n_prims; i++)
            if (d->prims[i].mesh == RSPT_MESH_SPHERE && d->prims[i].area_light != -1) s->has_sphere_light = true;
    }
    if (d->n_disks || d->n_cylinders) {   // ABI 27: every slot again with its kind
        const std::vector<QuadricDev> q = scene::quadric_slots(d);
        e = hipMemcpy(tris + 3 * d->n_prims, q.data(), q.size() * sizeof(QuadricDev), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(RSPT_E_HIP, "disk / cylinder records: %s", hipGetErrorString(e));
        s->has_spheres = s->has_quadrics = true;
        s->has_disks = d->n_disks != 0; s->has_cylinders = d->n_cylinders != 0;
        s->quadric_kinds = s->has_disks && s->has_cylinders ? "disk and cylinder" : (s->has_disks ? "disk" : "cylinder");
        if (f.disk_light || f.cylinder_light) {
            s->quadric_light_kinds = f.disk_light && f.cylinder_light ? "disk and cylinder" : (f.disk_light ? "disk" : "cylinder");
            s->quadric_light_what = f.disk_light && f.cylinder_light ? "disk area lights and cylinder area lights" : (f.disk_light ? "disk area lights" : "cylinder area lights");
        }
        s->shade_features |= SF_SPHERE | SF_QUADRIC;
    }
    s->dev.tris = tris;
    if (s->w4_ok && s->w4 && !f.instanced && (!s->has_alpha || s->alpha_simple) && env_size("RSPT_SERIAL_W4", 1) != 0) {   // the per-lane kernels' traversal (trace_serial.h)
        s->dev.w4 = s->w4; s->dev.w4_big = s->big_leaves; s->dev.w4_root = s->w4_root;
    }
    return RSPT_OK;
}

// InstDev records, and the keys of the moving instances
int upload_instances(rspt_scene_s* s, const rspt_scene_desc* d, const scene::W4Records& w4) {
    int rc;
    std::vector<InstDev> ins;
    std::vector<InstAnim> anims;
    scene::build_instances(d, w4.obj_root, &ins, &anims);
    if (!anims.empty()) {
        if (s->has_alpha && !s->w4_ok) return fail(RSPT_E_UNSUPPORTED, "moving object instances together with alpha-masked meshes in a scene whose records outgrow the four-box kernel");
        UP(anims, &s->dev.inst_anim);
        s->has_animated = true;
        s->shade_features |= SF_ANIM;
    }
    UP(ins, &s->dev.inst);
    s->dev.n_inst = d->n_instances;
    s->dev.inst_fixed = d->instancing_mode == RSPT_INSTANCING_FIXED ? 1u : 0u;
    return RSPT_OK;
}

}  // namespace

extern "C" {

int rspt_abi_version(void) { return RSPT_ABI_VERSION; }
// the shade-math mode: host-only state, no device needed (launch_trace.h g_shade_math; render_run.h picks the kernels)
int rspt_set_shade_math(uint32_t mode) {
    if (mode > RSPT_SHADE_MATH_FAST) return fail(RSPT_E_INVALID, "shade_math %u (0 exact, 1 fast)", mode);
    g_shade_math.store(mode);
    return RSPT_OK;
}
uint32_t rspt_get_shade_math(void) { return g_shade_math.load(); }
// the sphere-light gate: host-only state, no device needed (sphere_lights_mode above; rspt_light_distribution reads it at the call)
int rspt_set_sphere_lights(uint32_t on) {
    if (on > 1u) return fail(RSPT_E_INVALID, "sphere_lights = %u: 0 (off, the default) or 1 (on)", on);
    g_sphere_lights.store(on);
    return RSPT_OK;
}
int rspt_get_sphere_lights(void) { return (int)g_sphere_lights.load(); }
// the quadric-light gate: the same (quadric_lights_mode above)
int rspt_set_quadric_lights(uint32_t on) {
    if (on > 1u) return fail(RSPT_E_INVALID, "quadric_lights = %u: 0 (off, the default) or 1 (on)", on);
    g_quadric_lights.store(on);
    return RSPT_OK;
}
int rspt_get_quadric_lights(void) { return (int)g_quadric_lights.load(); }
// Replaces: BVHAccel::new (bvh.rs:96-392), on the device; see bvh_device.h
int64_t rspt_bvh_build_gpu(const float* P, uint64_t n_vertices, const uint32_t* tri_idx, uint64_t n_tris, uint32_t max_prims_in_node,
                           rspt_bvh_node* nodes_out, uint64_t nodes_cap, uint32_t* ordered_out) {
    using namespace rspt::bvhdev;
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (n_tris == 0) return 0;
    if (!P || !tri_idx || !nodes_out || !ordered_out) return fail(RSPT_E_INVALID, "null argument");
    if (n_tris > 0x3fffffffull) return fail(RSPT_E_UNSUPPORTED, "too many triangles");
    for (uint64_t i = 0; i < 3 * n_tris; i++)
        if (tri_idx[i] >= n_vertices) return fail(RSPT_E_INVALID, "vertex index out of range");
    HIP_TRY(hipSetDevice(g.device));
    const uint32_t n = (uint32_t)n_tris;
    const uint32_t max_prims = max_prims_in_node < 255 ? max_prims_in_node : 255;  // bvh.rs:102
    std::vector<void*> allocs;
    auto cleanup = [&]() { for (void* p : allocs) (void)hipFree(p); };
    auto dalloc = [&](size_t bytes) -> void* { void* p = nullptr; if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr; allocs.push_back(p); return p; };
#define BVD_ALLOC(var, type, count) type* var = (type*)dalloc(sizeof(type) * (size_t)(count)); if (!var) { cleanup(); return fail(RSPT_E_NOMEM, "hipMalloc failed in rspt_bvh_build_gpu"); }
    BVD_ALLOC(P_d, float, 3 * n_vertices)
    BVD_ALLOC(tri_d, uint32_t, 3 * (size_t)n)
    Prims pr[2];
    for (int s2 = 0; s2 < 2; s2++) {
        for (int a = 0; a < 3; a++) {
            BVD_ALLOC(lo, float, n) BVD_ALLOC(hi, float, n) BVD_ALLOC(cc, float, n)
            pr[s2].lo[a] = lo; pr[s2].hi[a] = hi; pr[s2].c[a] = cc;
        }
        BVD_ALLOC(pid, uint32_t, n) BVD_ALLOC(pnode, uint32_t, n)
        pr[s2].prim = pid; pr[s2].node = pnode;
    }
    BVD_ALLOC(nodes, Node, 2 * (size_t)n)
    BVD_ALLOC(level_nodes, uint32_t, 2 * (size_t)n + 2)
    BVD_ALLOC(buckets, Buckets, (size_t)n / 3 + 2)
    BVD_ALLOC(flag, uint32_t, n)
    BVD_ALLOC(scan, uint32_t, n)
    const uint32_t n_scan_blocks = (n + BVD_SCAN_BLOCK * BVD_SCAN_ITEMS - 1) / (BVD_SCAN_BLOCK * BVD_SCAN_ITEMS);
    BVD_ALLOC(block_sums, uint32_t, n_scan_blocks + 1)
    BVD_ALLOC(counters, uint32_t, 8)  // [0] node count, [1] next level size, [2] scan total
    BVD_ALLOC(ordered_d, uint32_t, n)
    BVD_ALLOC(out_d, rspt_bvh_node, 2 * (size_t)n)
#undef BVD_ALLOC
    hipStream_t st = g.stream;
    auto bail = [&](hipError_t e, const char* what) { cleanup(); return (int64_t)fail(RSPT_E_HIP, "%s: %s", what, hipGetErrorString(e)); };
    hipError_t e;
    if ((e = hipMemcpyAsync(P_d, P, sizeof(float) * 3 * n_vertices, hipMemcpyHostToDevice, st)) != hipSuccess) return bail(e, "upload P");
    if ((e = hipMemcpyAsync(tri_d, tri_idx, sizeof(uint32_t) * 3 * (size_t)n, hipMemcpyHostToDevice, st)) != hipSuccess) return bail(e, "upload indices");
    const uint32_t gp = (n + 255) / 256;
    hipLaunchKernelGGL(k_prim_info, dim3(gp), dim3(256), 0, st, P_d, tri_d, n, pr[0]);
    Node root{};
    root.start = 0; root.end = n; root.base = 0; root.child0 = root.child1 = BVD_NONE;
    const uint32_t zero = 0, one = 1;
    (void)hipMemcpyAsync(nodes, &root, sizeof root, hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(level_nodes, &zero, sizeof zero, hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(&counters[0], &one, sizeof one, hipMemcpyHostToDevice, st);
    std::vector<std::pair<uint32_t, uint32_t>> levels;  // (offset into level_nodes, count)
    uint32_t off = 0, n_level = 1;
    int cur = 0;
    while (n_level > 0) {
        if (levels.size() > 4096) { cleanup(); return fail(RSPT_E_UNSUPPORTED, "BVH deeper than 4096 levels"); }
        levels.push_back({off, n_level});
        const uint32_t* lv = level_nodes + off;
        const uint32_t gl = (n_level + 255) / 256;
        hipLaunchKernelGGL(k_node_reset, dim3(gl), dim3(256), 0, st, nodes, lv, n_level);
        hipLaunchKernelGGL(k_bounds, dim3(gp), dim3(256), 0, st, pr[cur], n, nodes);
        (void)hipMemsetAsync(&counters[3], 0, sizeof(uint32_t), st);
        hipLaunchKernelGGL(k_node_axis, dim3(gl), dim3(256), 0, st, nodes, lv, n_level, buckets, pr[cur], &counters[3]);
        hipLaunchKernelGGL(k_buckets, dim3(gp), dim3(256), 0, st, pr[cur], n, nodes, buckets);
        hipLaunchKernelGGL(k_split, dim3(gl), dim3(256), 0, st, nodes, lv, n_level, buckets, max_prims);
        hipLaunchKernelGGL(k_flags, dim3(gp), dim3(256), 0, st, pr[cur], n, nodes, flag, ordered_d);
        hipLaunchKernelGGL(k_scan_blocks, dim3(n_scan_blocks), dim3(BVD_SCAN_BLOCK), 0, st, flag, scan, block_sums, n);
        hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, st, block_sums, n_scan_blocks, &counters[2]);
        hipLaunchKernelGGL(k_scan_add, dim3(gp), dim3(256), 0, st, scan, block_sums, n);
        (void)hipMemsetAsync(&counters[1], 0, sizeof(uint32_t), st);
        uint32_t* next = level_nodes + off + n_level;
        hipLaunchKernelGGL(k_children, dim3(gl), dim3(256), 0, st, nodes, lv, n_level, scan, &counters[2], n, &counters[0], next, &counters[1]);
        hipLaunchKernelGGL(k_scatter, dim3(gp), dim3(256), 0, st, pr[cur], pr[cur ^ 1], n, nodes, flag, scan);
        uint32_t n_next = 0;
        if ((e = hipMemcpyAsync(&n_next, &counters[1], sizeof n_next, hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess) return bail(e, "bvh level");
        off += n_level;
        n_level = n_next;
        cur ^= 1;
    }
    uint32_t total = 0;
    if ((e = hipMemcpy(&total, &counters[0], sizeof total, hipMemcpyDeviceToHost)) != hipSuccess) return bail(e, "node count");
    if (total > nodes_cap) { cleanup(); return fail(RSPT_E_INVALID, "nodes_cap %llu < %u nodes", (unsigned long long)nodes_cap, total); }
    for (size_t l = levels.size(); l-- > 0;) hipLaunchKernelGGL(k_sizes, dim3((levels[l].second + 255) / 256), dim3(256), 0, st, nodes, level_nodes + levels[l].first, levels[l].second);
    for (size_t l = 0; l < levels.size(); l++) hipLaunchKernelGGL(k_indices, dim3((levels[l].second + 255) / 256), dim3(256), 0, st, nodes, level_nodes + levels[l].first, levels[l].second, out_d);
    if ((e = hipMemcpyAsync(nodes_out, out_d, sizeof(rspt_bvh_node) * total, hipMemcpyDeviceToHost, st)) != hipSuccess) return bail(e, "download nodes");
    if ((e = hipMemcpyAsync(ordered_out, ordered_d, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st)) != hipSuccess) return bail(e, "download order");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return bail(e, "bvh build");
    cleanup();
    return (int64_t)total;
}

const char* rspt_last_error(void) { return g_err.c_str(); }

int rspt_init(int32_t device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(RSPT_E_NODEVICE, "no HIP device: %s", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= n) return fail(RSPT_E_INVALID, "device %d out of range (have %d)", device, n);
    if (g.inited && g.device == device) return RSPT_OK;
    if (g.inited) rspt_shutdown();
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0 && !getenv("RSPT_ALLOW_ANY_ARCH"))
        return fail(RSPT_E_NODEVICE, "device %d is %s; librspt is built for gfx950 only", device, prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&g.stream2, hipStreamNonBlocking));
    HIP_TRY(hipHostMalloc((void**)&g.look, 8 * sizeof(QueueCounts), hipHostMallocDefault));
    g.device = device;
    g.n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    g.inited = true;
    return RSPT_OK;
}

void rspt_shutdown(void) {
    if (!g.inited) return;
    (void)rspt_comm_destroy();
    (void)hipSetDevice(g.device);
    (void)hipStreamSynchronize(g.stream);
    free_paths();
    void* ptrs[] = {g.dl.le_kind, g.dl.w_r, g.dl.w_t, g.dl.l_all, g.dl.ld_acc, g.dl.dim, g.dl.kidx, g.dl.nflags, g.dl.error, g.dl_queue, g.bin_keys, g.q_sorted, g.bin_info, g.hit_inst, g.cnt, g.ovf, g.spill, g.totals, g.sobol32, g.vdc, g.vdc_inv, g.filter_table, g.film_own, g.film_splat, g.film_out, g.pix_list, g.pix_index, g.primes, g.prime_sums, g.halton_perms, g.cam_anim, g.lens_elements, g.lens_bounds};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : g.events) (void)hipEventDestroy(e);
    if (g.look) (void)hipHostFree(g.look);
    (void)hipStreamDestroy(g.stream);
    (void)hipStreamDestroy(g.stream2);
    g = Ctx{};
}

int rspt_comm_unique_id(uint8_t id[RSPT_COMM_ID_BYTES]) {
    if (!id) return fail(RSPT_E_INVALID, "null argument");
    int rc = rccl_bind();
    if (rc) return rc;
    static_assert(sizeof(ncclUniqueId) == RSPT_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    RCCL_TRY(rc_.GetUniqueId(&u));
    memcpy(id, &u, sizeof u);
    return RSPT_OK;
}
const char* rspt_comm_library(void) {
    static std::string path;
    if (rccl_bind() != RSPT_OK) return nullptr;
    Dl_info info;
    if (path.empty()) path = (dladdr((void*)rc_.GetUniqueId, &info) && info.dli_fname) ? info.dli_fname : "(unknown)";
    return path.c_str();
}
int rspt_comm_init(int32_t rank, int32_t world, const uint8_t id[RSPT_COMM_ID_BYTES]) {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(RSPT_E_INVALID, "bad rank / world / id");
    int rc = rccl_bind();
    if (rc) return rc;
    if (rc_.comm) { (void)rc_.CommDestroy(rc_.comm); rc_.comm = nullptr; }
    HIP_TRY(hipSetDevice(g.device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    RCCL_TRY(rc_.CommInitRank(&rc_.comm, world, u, rank));
    rc_.rank = rank; rc_.world = world;
    if (!rc_.status) HIP_TRY(hipMalloc((void**)&rc_.status, sizeof(int32_t)));   // the status agreement's words (film_reduce_agree)
    if (!rc_.status_host) HIP_TRY(hipHostMalloc((void**)&rc_.status_host, sizeof(int32_t), hipHostMallocDefault));
    return RSPT_OK;
}
int rspt_comm_destroy(void) {
    if (rc_.comm) {
        if (g.inited) { (void)hipSetDevice(g.device); (void)hipStreamSynchronize(g.stream); }
        (void)rc_.CommDestroy(rc_.comm);
        rc_.comm = nullptr;
    }
    rc_.rank = rc_.world = 0;
    return RSPT_OK;
}

int rspt_scene_create(const rspt_scene_desc* d, rspt_scene_t* out) {
    using namespace rspt::scene;
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (!d || !out) return fail(RSPT_E_INVALID, "null argument");
    *out = nullptr;
    // ---- everything the host refuses or prepares before the device is touched (scene_validate.h, scene_materials.h): a bad scene must not fault the GPU ----
    SceneFacts facts;
    SceneMaterials sm;
    if (rspt_mat::Error e = prepare_scene(d, &facts, &sm)) return fail(e.code, "%s", e.text.c_str());
    const bool instanced = facts.instanced, quadrics = d->n_disks || d->n_cylinders;
    HIP_TRY(hipSetDevice(g.device));
    std::unique_ptr<rspt_scene_s> owner(new rspt_scene_s());   // an early return frees what was uploaded so far
    rspt_scene_s* s = owner.get();
    s->dev.time_div = 1u;
    s->has_null_material = facts.has_null || (instanced && d->instancing_mode == RSPT_INSTANCING_REFERENCE);  // instanced hits pass through like null surfaces (Q11)
    s->has_instances = instanced;
    s->has_alpha = facts.any_alpha;
    s->has_maplights = facts.has_maplights;
    s->maplight_kinds = facts.has_projection ? (facts.has_goniometric ? "projection and goniometric" : "projection") : (facts.has_goniometric ? "goniometric" : "");
    s->n_materials = d->n_materials;
    s->shade_features = sm.shade_features;
    s->shade_classes = sm.shade_classes;
    // ---- the caller's arrays, and what scene_records.h builds from them ----
    int rc;
    const rspt_bvh_node* nodes_d = nullptr;
    const rspt_mesh* meshes_d = nullptr;
    const float* P_d = nullptr;
    UP(d->nodes, d->n_nodes, &nodes_d);
    if (quadrics) UP(quadric_prims_as_sphere_slots(d), &s->dev.prims);
    else UP(d->prims, d->n_prims, &s->dev.prims);
    UP(d->meshes, d->n_meshes, &meshes_d);
    s->dev.meshes = meshes_d;
    if ((rc = upload_media(s, d))) return rc;
    UP(d->P, d->n_vertices * 3, &P_d);
    UP(d->N, d->N ? d->n_vertices * 3 : 0, &s->dev.N);
    UP(d->S, d->S ? d->n_vertices * 3 : 0, &s->dev.S);
    UP(d->UV, d->UV ? d->n_vertices * 2 : 0, &s->dev.UV);
    if (wants_tri_nuv(d) && d->n_prims * 80ull <= env_size("RSPT_TRI_NUV_MAX_BYTES", (size_t)16 << 30) && env_size("RSPT_TRI_NUV", 1) != 0) {   // (skipped beyond 16 GB)
        const float* dev_nuv = nullptr;
        UP(pack_tri_nuv(d), &dev_nuv);
        s->dev.tri_nuv = reinterpret_cast<const float4*>(dev_nuv);
    }
    if ((rc = upload_materials(s, d, sm))) return rc;
    UP(d->lights, d->n_lights, &s->dev.lights);
    if ((rc = upload_envmaps(s, d))) return rc;
    s->dev.nodes = reinterpret_cast<const float4*>(nodes_d);
    s->dev.n_nodes = (uint32_t)d->n_nodes; s->dev.n_prims = (uint32_t)d->n_prims; s->dev.n_lights = d->n_lights;
    if (d->n_nodes) {
        for (int i = 0; i < 3; i++) { s->dev.wb_min[i] = d->nodes[0].bmin[i]; s->dev.wb_max[i] = d->nodes[0].bmax[i]; }
    } else {
        for (int i = 0; i < 3; i++) { s->dev.wb_min[i] = RSPT_FLT_MAX; s->dev.wb_max[i] = -RSPT_FLT_MAX; }  // Bounds3f::default
    }
    const W4Records w4 = build_w4(d, facts);
    if ((rc = upload_w4(s, d, facts, w4))) return rc;
    if (d->n_prims && (rc = build_primitive_records(s, d, facts, w4, meshes_d, P_d))) return rc;
    if (instanced && (rc = upload_instances(s, d, w4))) return rc;
    if (d->n_nodes > 1 && !instanced) UP(build_pairs(d), &s->pairs);
    *out = owner.release();
    return RSPT_OK;
}
#undef UP

int rspt_scene_destroy(rspt_scene_t s) {
    if (!s) return RSPT_OK;
    if (g.inited) { (void)hipSetDevice(g.device); (void)hipStreamSynchronize(g.stream); }
    delete s;   // (its destructor frees the device arrays)
    return RSPT_OK;
}

namespace {
// A render that asked for the film reduce and failed before reaching it still takes part in the status agreement, so that the other
// ranks return RSPT_E_PEER instead of waiting for it; its own error code and message are kept.
int render_entry(rspt_scene_t s, const rspt_render_desc* d, float* film_host, void* film_dev, float* li_host, rspt_stats* stats) {
    rc_.status_exchanged = false;
    const int rc = (!film_host && !film_dev && !li_host) ? fail(RSPT_E_INVALID, "null output buffer") : render_impl(s, d, film_host, film_dev, li_host, stats);
    if (s && g.inited) { s->dev.ray_time = nullptr; s->dev.time_div = 1u; }   // the per-path times belong to the render that just ended (the buffer is the library's, not the scene's)
    if (rc != RSPT_OK && d && d->film_reduce && rc_.comm && g.inited && !rc_.status_exchanged) {
        const std::string kept = rspt_last_error();
        int32_t all = 0;
        (void)film_reduce_agree(1, &all);
        fail(rc, "%s", kept.c_str());
    }
    return rc;
}
}  // namespace

int rspt_render(rspt_scene_t s, const rspt_render_desc* d, float* film_xyzw, rspt_stats* stats) {
    return render_entry(s, d, film_xyzw, nullptr, nullptr, stats);
}
int rspt_render_device(rspt_scene_t s, const rspt_render_desc* d, void* film_dev, rspt_stats* stats) {
    return render_entry(s, d, nullptr, film_dev, nullptr, stats);
}
int rspt_render_samples(rspt_scene_t s, const rspt_render_desc* d, float* li_rgb, rspt_stats* stats) {
    return render_entry(s, d, nullptr, nullptr, li_rgb, stats);
}

int rspt_material_lobes(const rspt_scene_desc* desc, uint32_t material, uint32_t allow_multiple_lobes, rspt_material* out_material, rspt_bxdf out_bxdfs[8]) {
    if (!desc || !out_material || !out_bxdfs) return fail(RSPT_E_INVALID, "null argument");
    rspt_mat::Assembler as(desc, allow_multiple_lobes != 0);
    rspt_mat::Lobes lb;
    if (rspt_mat::Error e = as.assemble(material, &lb)) return fail(e.code, "%s", e.text.c_str());
    *out_material = lb.mat;
    if (lb.dynamic) return RSPT_MATERIAL_DYNAMIC;
    for (size_t i = 0; i < lb.lobes.size(); i++) out_bxdfs[i] = lb.lobes[i];
    return (int)lb.lobes.size();
}

int rspt_camera_decompose(const float start_m[16], float start_time, const float end_m[16], float end_time, int32_t* animated_out, float trs_out[46]) {
    if (!start_m || !end_m || !animated_out || !trs_out) return fail(RSPT_E_INVALID, "null argument");
    CamAnim ca;
    *animated_out = camanim::camera_keys(start_m, start_time, end_m, end_time, &ca) ? 1 : 0;
    if (*animated_out) {
        memcpy(trs_out, ca.t, sizeof ca.t);
        memcpy(trs_out + 6, ca.r, sizeof ca.r);
        memcpy(trs_out + 14, ca.s, sizeof ca.s);
    }
    return RSPT_OK;
}
// RealisticCamera::new (realistic.rs:50-144) up to the state it builds, over the host side of dev_lens.h.  focus_binary_search (:92) is left out: the
// reference discards its result (`_fb`) and it changes no state.
int rspt_realistic_camera_setup(const float* lens_data, uint32_t n_elements, float aperture_diameter_mm, float focus_distance, float film_diagonal_mm,
                                uint32_t n_bounds, rspt_lens_element* elements_out, float* bounds_out, int32_t n_threads) {
    if (!lens_data || !elements_out || !bounds_out) return fail(RSPT_E_INVALID, "null argument");
    if (n_elements == 0 || n_elements > RSPT_MAX_LENS_ELEMENTS) return fail(RSPT_E_INVALID, "n_elements must be in [1, %d]", RSPT_MAX_LENS_ELEMENTS);
    if (n_bounds == 0 || n_bounds > (1u << 16)) return fail(RSPT_E_INVALID, "n_bounds must be in [1, 65536]");
    std::vector<rspt_lens_element> el(n_elements);
    for (uint32_t i = 0; i < n_elements; i++) {   // :61-80: mm -> m; a stop takes the given aperture unless that exceeds the file's ("Clamping it.")
        const float* q = lens_data + 4 * (size_t)i;
        float diameter = q[3];
        if (q[0] == 0.0f && !(aperture_diameter_mm > q[3])) diameter = aperture_diameter_mm;
        el[i] = rspt_lens_element{q[0] * 0.001f, q[1] * 0.001f, q[2], diameter * 0.001f / 2.0f};
    }
    const float diagonal = film_diagonal_mm * 0.001f;   // Film::new (film.rs:214)
    uint32_t t_neg = 0;
    // focus_thick_lens (:483-499) over compute_thick_lens_approximation (:444-482) and compute_cardinal_points (:431-443)
    float pz[2], fz[2];
    {
        const float x = 0.001f * diagonal;
        auto cardinal = [&](const LensRay& r_in, const LensRay& r_out, int idx) {
            const float tf = -r_out.o.x / r_out.d.x;
            fz[idx] = -(r_out.o.z + r_out.d.z * tf);
            const float tp = (r_in.o.x - r_out.o.x) / r_out.d.x;
            pz[idx] = -(r_out.o.z + r_out.d.z * tp);
        };
        LensRay r_scene{lv3{x, 0.0f, lens_front_z(el.data(), n_elements) + 1.0f}, lv3{0.0f, 0.0f, -1.0f}, RSPT_INF}, r_film{};
        if (!lens_trace_from_scene(el.data(), n_elements, r_scene, &r_film, &t_neg))
            return fail(RSPT_E_INVALID, "Unable to trace ray from scene to film for thick lens approximation. Is aperture stop extremely small?");
        cardinal(r_scene, r_film, 0);
        r_film.o = lv3{x, 0.0f, el.back().thickness - 1.0f};
        r_film.d = lv3{0.0f, 0.0f, 1.0f};
        if (!lens_trace_from_film(el.data(), n_elements, r_film, &r_scene, &t_neg))
            return fail(RSPT_E_INVALID, "Unable to trace ray from film to scene for thick lens approximation. Is aperture stop extremely small?");
        cardinal(r_film, r_scene, 1);
    }
    const float f = fz[0] - pz[0], z = -focus_distance;
    const float c = (pz[1] - z - pz[0]) * (pz[1] - z - 4.0f * f - pz[0]);
    if (!(c > 0.0f))
        return fail(RSPT_E_INVALID, "Coefficient must be positive. It looks focus_distance: %g is too short for a given lenses configuration", (double)focus_distance);
    const float delta = 0.5f * (pz[1] - z + pz[0] - std::sqrt(c));
    el.back().thickness = el.back().thickness + delta;
    // bound_exit_pupil over the bands of half the diagonal (:100-139); a band's box is a min / max over the points that pass, so the split over threads cannot show
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned nt = std::max(1u, std::min({16u, n_threads > 0 ? (unsigned)n_threads : hw, n_bounds}));
    std::atomic<uint32_t> next{0}, neg{0};
    auto worker = [&]() {
        uint32_t tn = 0;
        for (;;) {
            const uint32_t i = next.fetch_add(1);
            if (i >= n_bounds) break;
            const float r0 = (float)i / (float)n_bounds * diagonal / 2.0f, r1 = (float)(i + 1u) / (float)n_bounds * diagonal / 2.0f;
            lens_bound_exit_pupil(el.data(), n_elements, r0, r1, bounds_out + 4 * (size_t)i, &tn);
        }
        neg += tn;
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();
    if (t_neg + neg.load()) return fail(RSPT_E_INVALID, "assertion failed: t >= 0.0 (a lens interface was met behind the ray's origin, %u times)", t_neg + neg.load());
    memcpy(elements_out, el.data(), n_elements * sizeof(rspt_lens_element));
    return RSPT_OK;
}

int rspt_camera_rays(const rspt_render_desc* d, const float* samples, uint64_t n, float* out) {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (!d || (n && (!samples || !out))) return fail(RSPT_E_INVALID, "null argument");
    if (int rc = validate_camera(d)) return rc;
    if (d->camera_kind != RSPT_CAMERA_REALISTIC) return fail(RSPT_E_UNSUPPORTED, "rspt_camera_rays serves camera_kind 3 (realistic) only");
    if (n == 0) return RSPT_OK;
    if (n > (1ull << 28)) return fail(RSPT_E_INVALID, "more than 2^28 camera samples in one call");
    HIP_TRY(hipSetDevice(g.device));
    int rc;
    RenderDev rd{};
    memcpy(rd.camera_to_world, d->camera_to_world, sizeof rd.camera_to_world);
    rd.camera_kind = d->camera_kind; rd.full_res[0] = d->full_res[0]; rd.full_res[1] = d->full_res[1];
    rd.shutter_open = d->shutter_open; rd.shutter_close = d->shutter_close;
    rd.spp = d->spp;
    if (d->camera_animated) {
        CamAnim ca;
        if (camanim::camera_keys(d->camera_to_world, d->camera_time[0], d->camera_to_world_end, d->camera_time[1], &ca)) {
            if (!g.cam_anim && (rc = dev_alloc(&g.cam_anim, 1))) return rc;
            HIP_TRY(hipMemcpy(g.cam_anim, &ca, sizeof ca, hipMemcpyHostToDevice));
            rd.cam_anim = g.cam_anim;
        }
    }
    LensSystem lens;
    if ((rc = upload_lens(d, &lens))) return rc;
    DevTemps temps;
    float *smp_dev = nullptr, *out_dev = nullptr;
    if ((rc = dev_alloc(&smp_dev, 5 * n))) return rc;
    temps.p.push_back(smp_dev);
    if ((rc = dev_alloc(&out_dev, 22 * n))) return rc;
    temps.p.push_back(out_dev);
    HIP_TRY(hipMemcpyAsync(smp_dev, samples, 5 * n * sizeof(float), hipMemcpyHostToDevice, g.stream));
    hipLaunchKernelGGL(k_camera_rays, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, g.stream, rd, lens, smp_dev, n, out_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, out_dev, 22 * n * sizeof(float), hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return RSPT_OK;
}

int rspt_motion_bounds(const float start_m[16], float start_time, const float end_m[16], float end_time, const float box_min[3], const float box_max[3],
                       float out_min[3], float out_max[3], int32_t* flags_out) {
    if (!start_m || !end_m || !box_min || !box_max || !out_min || !out_max) return fail(RSPT_E_INVALID, "null argument");
    for (int i = 0; i < 16; i++) if (!std::isfinite(start_m[i]) || !std::isfinite(end_m[i])) return fail(RSPT_E_INVALID, "non-finite key matrix");
    for (int i = 0; i < 3; i++) if (!std::isfinite(box_min[i]) || !std::isfinite(box_max[i])) return fail(RSPT_E_INVALID, "non-finite box");
    if (!std::isfinite(start_time) || !std::isfinite(end_time)) return fail(RSPT_E_INVALID, "non-finite key time");
    motion::Keys keys;
    motion::make_keys(start_m, start_time, end_m, end_time, &keys);
    motion::Box b;
    for (int i = 0; i < 3; i++) { b.lo[i] = box_min[i]; b.hi[i] = box_max[i]; }
    bool overflow = false;
    const motion::Box r = motion::motion_bounds(keys, b, &overflow);
    if (overflow) return fail(RSPT_E_UNSUPPORTED, "more than eight motion-derivative zeros for one point: the reference's interval_find_zeros indexes past its array here (transform.rs:2346)");
    for (int i = 0; i < 3; i++) { out_min[i] = r.lo[i]; out_max[i] = r.hi[i]; }
    if (flags_out) *flags_out = (keys.animated ? 1 : 0) | (keys.has_rotation ? 2 : 0);
    return RSPT_OK;
}
}  // extern "C" (reopened below)
namespace {
// stage hook rspt_libm, codes 8 .. 12: the device's traversal / shading geometry AS THE KERNELS CALL IT, one element = 16 floats in, 16 floats out (include/rspt.h) —
// what tests/golden/geom_functions.npz pins by the reference's own text
__global__ void k_leaf_geom(uint32_t fn, const float* __restrict__ x, uint64_t n, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a[16], r[16];
#pragma unroll
    for (int k = 0; k < 16; k++) { a[k] = x[16 * i + k]; r[k] = 0.0f; }
    if (fn == RSPT_LIBM_TRIANGLE) {              // Triangle::intersect's watertight test: ray_shear once per ray + tri_test per triangle (dev_scene.h), as traverse<> / k_trace_w4 run it
        const f3 d{a[12], a[13], a[14]};
        const RayShear rs = ray_shear(d);
        float t = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
        const bool hit = tri_test(f3{a[0], a[1], a[2]}, f3{a[3], a[4], a[5]}, f3{a[6], a[7], a[8]}, f3{a[9], a[10], a[11]}, rs, a[15], &t, &b0, &b1, &b2);
        r[0] = hit ? 1.0f : 0.0f; r[1] = hit ? t : 0.0f; r[2] = hit ? b0 : 0.0f; r[3] = hit ? b1 : 0.0f; r[4] = hit ? b2 : 0.0f;
    } else if (fn == RSPT_LIBM_BOX) {            // Bounds3f::intersect_p: k_trace's box_hit (kernels.h), and k_trace_w4's choice (trace_w4.h): the pair form for finite reciprocals, else the literal chain
        const f3 o{a[6], a[7], a[8]}, inv{a[9], a[10], a[11]};
        const bool n0 = a[12] != 0.0f, n1 = a[13] != 0.0f, n2 = a[14] != 0.0f;
        r[0] = box_hit(float4{a[0], a[1], a[2], a[3]}, float4{a[4], a[5], 0.0f, 0.0f}, o, inv, n0, n1, n2, a[15]) ? 1.0f : 0.0f;
        if (fabsf(inv.x) < RSPT_INF && fabsf(inv.y) < RSPT_INF && fabsf(inv.z) < RSPT_INF) {
            bool h0, h1; float m0, m1;
            box_pair_hit_m(float4{a[0], a[0], a[3], a[3]}, float4{a[1], a[1], a[4], a[4]}, float4{a[2], a[2], a[5], a[5]}, o.x, o.y, o.z, inv.x, inv.y, inv.z, a[15], &h0, &h1, &m0, &m1);
            r[1] = h0 ? 1.0f : 0.0f; r[2] = h1 ? 1.0f : 0.0f; r[3] = 1.0f;
        } else {
            float m0;
            r[1] = r[2] = box_hit6_m(a[0], a[1], a[2], a[3], a[4], a[5], o, inv, n0, n1, n2, a[15], &m0) ? 1.0f : 0.0f; r[3] = 0.0f;
        }
    } else if (fn == RSPT_LIBM_OFFSET_RAY_ORIGIN) {   // pnt3_offset_ray_origin (dev_math.h): every spawned ray
        const f3 po = offset_ray_origin(f3{a[0], a[1], a[2]}, f3{a[3], a[4], a[5]}, f3{a[6], a[7], a[8]}, f3{a[9], a[10], a[11]});
        r[0] = po.x; r[1] = po.y; r[2] = po.z;
    } else if (fn == RSPT_LIBM_MICROFACET) {     // TrowbridgeReitzDistribution::d / lambda / g1 / g / pdf (dev_bsdf.h)
        const f3 wo{a[0], a[1], a[2]}, wh{a[3], a[4], a[5]};
        r[0] = tr_d(a[6], a[7], wh); r[1] = tr_lambda(a[6], a[7], wo); r[2] = tr_g1(a[6], a[7], wo); r[3] = tr_g(a[6], a[7], wo, wh); r[4] = tr_pdf(a[6], a[7], wo, wh);
    } else if (fn == RSPT_LIBM_AREA_LIGHT) {     // DiffuseAreaLight::sample_li on one emitting triangle without vertex normals (dev_scene.h light_sample_li / tri_sample_ref), radiance (1, 1, 1)
        SceneDev sc{};
        TriRec t; t.p0 = f3{a[0], a[1], a[2]}; t.p1 = f3{a[3], a[4], a[5]}; t.p2 = f3{a[6], a[7], a[8]}; t.material = 0; t.area_light = 0;
        const uint32_t fl = (uint32_t)a[14];
        t.flags = (fl & 2u) ? MF_FLIP : 0u;
        rspt_light lt{}; lt.kind = RSPT_LIGHT_DIFFUSE_AREA; lt.prim = 0; lt.L[0] = lt.L[1] = lt.L[2] = 1.0f; lt.two_sided = (fl & 4u) ? 1u : 0u;
        f3 wi{0.0f, 0.0f, 0.0f}; float pdf = 0.0f; LightSample ls; ls.p = ls.p_err = ls.n = f3{0.0f, 0.0f, 0.0f};
        const rgb li = light_sample_li(sc, lt, f3{a[9], a[10], a[11]}, f2{a[12], a[13]}, &wi, &pdf, &ls, &t);
        r[0] = pdf; r[1] = pdf == 0.0f ? 0.0f : wi.x; r[2] = pdf == 0.0f ? 0.0f : wi.y; r[3] = pdf == 0.0f ? 0.0f : wi.z; r[4] = pdf == 0.0f ? 0.0f : li.r;
        r[5] = ls.p.x; r[6] = ls.p.y; r[7] = ls.p.z; r[8] = ls.n.x; r[9] = ls.n.y; r[10] = ls.n.z; r[11] = ls.p_err.x; r[12] = ls.p_err.y; r[13] = ls.p_err.z;
    } else {                                     // RSPT_LIBM_VECTORS: vec3_cross_vec3, vec3_coordinate_system, refract, cosine_sample_hemisphere (dev_math.h, dev_bsdf.h)
        const f3 u{a[0], a[1], a[2]}, v{a[3], a[4], a[5]};
        const f3 c = cross(u, v);
        f3 v2{0.0f, 0.0f, 0.0f}, v3{0.0f, 0.0f, 0.0f}, wt{0.0f, 0.0f, 0.0f};
        coordinate_system(u, &v2, &v3);
        const bool ok = refract(u, v, a[6], &wt);
        const f3 h = cosine_hemisphere(f2{a[7], a[8]});
        r[0] = c.x; r[1] = c.y; r[2] = c.z; r[3] = v2.x; r[4] = v2.y; r[5] = v2.z; r[6] = v3.x; r[7] = v3.y; r[8] = v3.z;
        r[9] = ok ? wt.x : 0.0f; r[10] = ok ? wt.y : 0.0f; r[11] = ok ? wt.z : 0.0f; r[12] = ok ? 1.0f : 0.0f; r[13] = h.x; r[14] = h.y; r[15] = h.z;
    }
#pragma unroll
    for (int k = 0; k < 16; k++) out[16 * i + k] = r[k];
}
// rspt_libm code 14: one lobe record (the 116 bytes of an rspt_bxdf, as 29 floats) + wo, wi, u -> lobe_f, lobe_pdf, lobe_sample_f (dev_bsdf.h) as the shade kernels call them;
// 48 floats in, 48 floats out per element
__global__ void k_leaf_lobe(const float* __restrict__ x, uint64_t n, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rspt_bxdf b;
    static_assert(sizeof(rspt_bxdf) == 116, "rspt_bxdf is 29 words");
    uint32_t* bw = reinterpret_cast<uint32_t*>(&b);
    for (int k = 0; k < 29; k++) bw[k] = __float_as_uint(x[48 * i + k]);
    const float* q = x + 48 * i + 29;
    const f3 wo{q[0], q[1], q[2]}, wi{q[3], q[4], q[5]};
    const LobeTex lt{nullptr, 0};
    float* o = out + 48 * i;
    for (int k = 0; k < 48; k++) o[k] = 0.0f;
    const rgb f = lobe_f<SF_ALL>(b, lt, wo, wi);
    o[0] = f.r; o[1] = f.g; o[2] = f.b; o[3] = lobe_pdf<SF_ALL>(b, lt, wo, wi);
    f3 w{0.0f, 0.0f, 0.0f}; float pdf = 0.0f; uint32_t st = 255u;
    const rgb sf = lobe_sample_f<SF_ALL>(b, lt, wo, &w, f2{q[6], q[7]}, &pdf, &st, true);
    o[4] = sf.r; o[5] = sf.g; o[6] = sf.b; o[7] = w.x; o[8] = w.y; o[9] = w.z; o[10] = pdf; o[11] = (float)st; o[12] = (float)lobe_type(b.type);
}
// rspt_libm code 15 (ABI 23): one rspt_sphere (42 words) + o, d, t_max -> sphere_hit and sphere_test (dev_sphere.h) as the traversal calls them; 64 floats in and out
__global__ void k_leaf_sphere(const float* __restrict__ x, uint64_t n, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rspt_sphere sp;
    uint32_t* sw = reinterpret_cast<uint32_t*>(&sp);
    for (int k = 0; k < 42; k++) sw[k] = __float_as_uint(x[64 * i + k]);
    const float* q = x + 64 * i + 42;
    const f3 o{q[0], q[1], q[2]}, d{q[3], q[4], q[5]};
    float* r = out + 64 * i;
    for (int k = 0; k < 64; k++) r[k] = 0.0f;
    SphereHit h;
    if (sphere_hit(sp, o, d, q[6], &h)) {
        const f3 v[13] = {h.p, h.p_error, h.n, f3{h.u, h.v, 0.0f}, h.dpdu, h.dpdv, h.dndu, h.dndv, h.sn, h.sdpdu, h.sdpdv, h.sdndu, h.sdndv};
        r[0] = 1.0f; r[1] = h.t;
        int k = 2;
        for (int j = 0; j < 13; j++) {
            r[k++] = v[j].x; r[k++] = v[j].y;
            if (j != 3) r[k++] = v[j].z;
        }
    }
    float t = 0.0f;
    r[43] = sphere_test(sp, o, d, q[6], &t) ? 1.0f : 0.0f;
}
// rspt_quadric_intersect (ABI 27): one rspt_sphere / rspt_disk / rspt_cylinder + o, d, t_max -> quadric_hit and quadric_test (dev_quadric.h) as the quadric
// instantiations call them; 64 floats in and out, in k_leaf_sphere's layout
__global__ void k_leaf_quadric(uint32_t kind, uint32_t n_words, const float* __restrict__ x, uint64_t n, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    QuadricDev qd;
    uint32_t* sw = reinterpret_cast<uint32_t*>(&qd);
    for (uint32_t k = 0; k < 44u; k++) sw[k] = k < n_words ? __float_as_uint(x[64 * i + k]) : 0u;
    qd.kind = kind;
    const float* q = x + 64 * i + n_words;
    const f3 o{q[0], q[1], q[2]}, d{q[3], q[4], q[5]};
    float* r = out + 64 * i;
    for (int k = 0; k < 64; k++) r[k] = 0.0f;
    SphereHit h;
    if (quadric_hit(qd, o, d, q[6], &h)) {
        const f3 v[13] = {h.p, h.p_error, h.n, f3{h.u, h.v, 0.0f}, h.dpdu, h.dpdv, h.dndu, h.dndv, h.sn, h.sdpdu, h.sdpdv, h.sdndu, h.sdndv};
        r[0] = 1.0f; r[1] = h.t;
        int k = 2;
        for (int j = 0; j < 13; j++) {
            r[k++] = v[j].x; r[k++] = v[j].y;
            if (j != 3) r[k++] = v[j].z;
        }
    }
    float t = 0.0f;
    r[43] = quadric_test(qd, o, d, q[6], &t) ? 1.0f : 0.0f;
}
// rspt_sphere_light: one rspt_sphere (42 words), a flags word (non-zero: two-sided), the reference point's p, p_error, n, u[2] and a query direction wi ->
// Sphere::area / sample / sample_with_ref_point / pdf_with_ref_point and DiffuseAreaLight::sample_li of L = 1 (dev_sphere_light.h); 64 floats in and out
__global__ void k_sphere_light(const float* __restrict__ x, uint64_t n, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rspt_sphere sp;
    uint32_t* sw = reinterpret_cast<uint32_t*>(&sp);
    for (int k = 0; k < 42; k++) sw[k] = __float_as_uint(x[64 * i + k]);
    const float* q = x + 64 * i + 42;
    rspt_light lt{};
    lt.kind = RSPT_LIGHT_DIFFUSE_AREA;
    lt.L[0] = lt.L[1] = lt.L[2] = 1.0f;
    lt.two_sided = __float_as_uint(q[0]) != 0u;
    const SlRef ref{f3{q[1], q[2], q[3]}, f3{q[4], q[5], q[6]}, f3{q[7], q[8], q[9]}};
    const f2 u{q[10], q[11]};
    const f3 wq{q[12], q[13], q[14]};
    float* r = out + 64 * i;
    for (int k = 0; k < 64; k++) r[k] = 0.0f;
    r[0] = sphere_area(sp);
    float pdf = 0.0f;
    LightSample a = sphere_sample(sp, u, &pdf);
    r[1] = a.p.x; r[2] = a.p.y; r[3] = a.p.z; r[4] = a.p_err.x; r[5] = a.p_err.y; r[6] = a.p_err.z; r[7] = a.n.x; r[8] = a.n.y; r[9] = a.n.z; r[10] = pdf;
    pdf = 0.0f;
    a = sphere_sample_ref(sp, ref, u, &pdf);
    r[11] = a.p.x; r[12] = a.p.y; r[13] = a.p.z; r[14] = a.p_err.x; r[15] = a.p_err.y; r[16] = a.p_err.z; r[17] = a.n.x; r[18] = a.n.y; r[19] = a.n.z; r[20] = pdf;
    pdf = 0.0f;
    f3 wi{0.0f, 0.0f, 0.0f};
    const rgb li = sphere_light_sample_li(sp, lt, ref, u, &wi, &pdf, &a);
    r[21] = li.r; r[22] = li.g; r[23] = li.b; r[24] = wi.x; r[25] = wi.y; r[26] = wi.z; r[27] = pdf;
    r[28] = sphere_pdf_ref(sp, ref, wq);
}
// rspt_quadric_light: one rspt_disk or rspt_cylinder (40 words), its kind (the BITS of RSPT_MESH_DISK / RSPT_MESH_CYLINDER), a flags word (non-zero: two-sided),
// the reference point's p, p_error, n, u[2] and a query direction wi -> area / sample / sample_with_ref_point / pdf_with_ref_point of the shape and
// DiffuseAreaLight::sample_li / power of L = 1 (dev_quadric_light.h); 64 floats in and out.  Any other kind: all words 0.
__global__ void k_quadric_light(const float* __restrict__ x, uint64_t n, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    QuadricDev qd;
    uint32_t* qw = reinterpret_cast<uint32_t*>(&qd);
    for (int k = 0; k < (int)(sizeof(QuadricDev) / 4); k++) qw[k] = 0u;
    for (int k = 0; k < 40; k++) qw[k] = __float_as_uint(x[64 * i + k]);
    const uint32_t kind = __float_as_uint(x[64 * i + 40]);
    qd.kind = kind == RSPT_MESH_DISK ? QK_DISK : QK_CYLINDER;
    const float* q = x + 64 * i + 42;
    rspt_light lt{};
    lt.kind = RSPT_LIGHT_DIFFUSE_AREA;
    lt.L[0] = lt.L[1] = lt.L[2] = 1.0f;
    lt.two_sided = __float_as_uint(q[0]) != 0u;
    const SlRef ref{f3{q[1], q[2], q[3]}, f3{q[4], q[5], q[6]}, f3{q[7], q[8], q[9]}};
    const f2 u{q[10], q[11]};
    const f3 wq{q[12], q[13], q[14]};
    float* r = out + 64 * i;
    for (int k = 0; k < 64; k++) r[k] = 0.0f;
    if (kind != RSPT_MESH_DISK && kind != RSPT_MESH_CYLINDER) return;
    r[0] = quadric_area(qd);
    float pdf = 0.0f;
    LightSample a = quadric_sample(qd, u, &pdf);
    r[1] = a.p.x; r[2] = a.p.y; r[3] = a.p.z; r[4] = a.p_err.x; r[5] = a.p_err.y; r[6] = a.p_err.z; r[7] = a.n.x; r[8] = a.n.y; r[9] = a.n.z; r[10] = pdf;
    pdf = 0.0f;
    a = quadric_sample_ref(qd, ref, u, &pdf);
    r[11] = a.p.x; r[12] = a.p.y; r[13] = a.p.z; r[14] = a.p_err.x; r[15] = a.p_err.y; r[16] = a.p_err.z; r[17] = a.n.x; r[18] = a.n.y; r[19] = a.n.z; r[20] = pdf;
    pdf = 0.0f;
    f3 wi{0.0f, 0.0f, 0.0f};
    const rgb li = quadric_light_sample_li(qd, lt, ref, u, &wi, &pdf, &a);
    r[21] = li.r; r[22] = li.g; r[23] = li.b; r[24] = wi.x; r[25] = wi.y; r[26] = wi.z; r[27] = pdf;
    r[28] = quadric_pdf_ref(qd, ref, wq);
    const rgb pw = quadric_light_power(qd, lt);
    r[29] = pw.r; r[30] = pw.g; r[31] = pw.b;
}
}  // namespace
extern "C" {
int rspt_quadric_light(const float* x, uint64_t n, float* out) {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (n == 0) return RSPT_OK;
    if (!x || !out || n > (1ull << 25)) return fail(RSPT_E_INVALID, "null argument or more than 2^25 elements");
    HIP_TRY(hipSetDevice(g.device));
    float *xd = nullptr, *od = nullptr;
    struct Guard { float **a, **b; ~Guard() { for (float** p : {a, b}) if (*p) (void)hipFree(*p); } } guard{&xd, &od};
    int rc;
    if ((rc = dev_alloc(&xd, n * 64)) || (rc = dev_alloc(&od, n * 64))) return rc;
    HIP_TRY(hipMemcpyAsync(xd, x, n * 64 * sizeof(float), hipMemcpyHostToDevice, g.stream));
    hipLaunchKernelGGL(k_quadric_light, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, g.stream, xd, n, od);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, od, n * 64 * sizeof(float), hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return RSPT_OK;
}

int rspt_sphere_light(const float* x, uint64_t n, float* out) {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (n == 0) return RSPT_OK;
    if (!x || !out || n > (1ull << 25)) return fail(RSPT_E_INVALID, "null argument or more than 2^25 elements");
    HIP_TRY(hipSetDevice(g.device));
    float *xd = nullptr, *od = nullptr;
    struct Guard { float **a, **b; ~Guard() { for (float** p : {a, b}) if (*p) (void)hipFree(*p); } } guard{&xd, &od};
    int rc;
    if ((rc = dev_alloc(&xd, n * 64)) || (rc = dev_alloc(&od, n * 64))) return rc;
    HIP_TRY(hipMemcpyAsync(xd, x, n * 64 * sizeof(float), hipMemcpyHostToDevice, g.stream));
    hipLaunchKernelGGL(k_sphere_light, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, g.stream, xd, n, od);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, od, n * 64 * sizeof(float), hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return RSPT_OK;
}

int rspt_quadric_intersect(uint32_t shape, const float* x, uint64_t n, float* out) {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (shape != RSPT_MESH_SPHERE && shape != RSPT_MESH_DISK && shape != RSPT_MESH_CYLINDER) return fail(RSPT_E_INVALID, "bad shape %#x (RSPT_MESH_SPHERE, RSPT_MESH_DISK, RSPT_MESH_CYLINDER)", shape);
    if (n == 0) return RSPT_OK;
    if (!x || !out || n > (1ull << 25)) return fail(RSPT_E_INVALID, "null argument or more than 2^25 elements");
    HIP_TRY(hipSetDevice(g.device));
    float *xd = nullptr, *od = nullptr;
    struct Guard { float **a, **b; ~Guard() { for (float** p : {a, b}) if (*p) (void)hipFree(*p); } } guard{&xd, &od};
    int rc;
    if ((rc = dev_alloc(&xd, n * 64)) || (rc = dev_alloc(&od, n * 64))) return rc;
    HIP_TRY(hipMemcpyAsync(xd, x, n * 64 * sizeof(float), hipMemcpyHostToDevice, g.stream));
    const uint32_t kind = shape == RSPT_MESH_SPHERE ? QK_SPHERE : (shape == RSPT_MESH_DISK ? QK_DISK : QK_CYLINDER);
    hipLaunchKernelGGL(k_leaf_quadric, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, g.stream, kind, kind == QK_SPHERE ? 42u : 40u, xd, n, od);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, od, n * 64 * sizeof(float), hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return RSPT_OK;
}

int rspt_libm(uint32_t fn, const float* x, const float* y, uint64_t n, float* out) {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (n == 0) return RSPT_OK;
    if (fn > RSPT_LIBM_SPHERE || !x || !out || (fn == RSPT_LIBM_ATAN2 && !y) || n > (fn >= RSPT_LIBM_MAT4_INVERSE ? (1ull << 27) : (1ull << 31))) return fail(RSPT_E_INVALID, "bad function, null argument or more than 2^31 values (2^27 sixteen-float elements)");
    HIP_TRY(hipSetDevice(g.device));
    float *xd = nullptr, *yd = nullptr, *od = nullptr;
    struct Guard { float **a, **b, **c; ~Guard() { for (float** p : {a, b, c}) if (*p) (void)hipFree(*p); } } guard{&xd, &yd, &od};
    int rc;
    const uint64_t per = fn == RSPT_LIBM_SPHERE ? 64u : (fn == RSPT_LIBM_LOBE ? 48u : (fn >= RSPT_LIBM_MAT4_INVERSE ? 16u : 1u));   // values per element
    if ((rc = dev_alloc(&xd, n * per)) || (rc = dev_alloc(&od, n * per)) || (y && (rc = dev_alloc(&yd, n)))) return rc;
    HIP_TRY(hipMemcpyAsync(xd, x, n * per * sizeof(float), hipMemcpyHostToDevice, g.stream));
    if (y) HIP_TRY(hipMemcpyAsync(yd, y, n * sizeof(float), hipMemcpyHostToDevice, g.stream));
    if (fn == RSPT_LIBM_SPHERE) hipLaunchKernelGGL(k_leaf_sphere, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, g.stream, xd, n, od);
    else if (fn == RSPT_LIBM_LOBE) hipLaunchKernelGGL(k_leaf_lobe, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, g.stream, xd, n, od);
    else if (fn > RSPT_LIBM_MAT4_INVERSE) hipLaunchKernelGGL(k_leaf_geom, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, g.stream, fn, xd, n, od);
    else hipLaunchKernelGGL(k_libm, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, g.stream, fn, xd, yd, n, od);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, od, n * per * sizeof(float), hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return RSPT_OK;
}

int rspt_light_distribution(rspt_scene_t s, uint32_t strategy, const float p[3], float* func_out, float* cdf_out, int32_t nvox_out[3], int32_t voxel_out[3]) {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (!s || !p || !func_out || !cdf_out) return fail(RSPT_E_INVALID, "null argument");
    // (a scene whose spheres are no lights needs no sphere code here: the spatial voxels take the world bound from the BVH root, which holds the spheres)
    bool ql_on = false;
    if (s->quadric_light_kinds) {   // served while the quadric-light gate is on (rspt_set_quadric_lights) by the _ql kernels; off: today's answer
        const int ql = quadric_lights_mode();
        if (ql < 0) return fail(RSPT_E_INVALID, "RSPT_QUADRIC_LIGHTS=%s: 0 or 1", getenv("RSPT_QUADRIC_LIGHTS"));
        if (!ql) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive %s: the light distributions are not built for %s yet", s->quadric_light_kinds, s->quadric_light_what);
        ql_on = true;
    }
    if (s->has_sphere_light && s->has_quadrics) {   // an emissive sphere in a scene with a disk or a cylinder: served by the _ql kernels while BOTH gates are on
        const int sl = sphere_lights_mode();
        if (sl < 0) return fail(RSPT_E_INVALID, "RSPT_SPHERE_LIGHTS=%s: 0 or 1", getenv("RSPT_SPHERE_LIGHTS"));
        const int ql = ql_on ? 1 : quadric_lights_mode();
        if (!sl && ql == 1) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere next to a %s: a sphere area light there needs the sphere-light gate too (rspt_set_sphere_lights)", s->quadric_kinds);
        if (!sl) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere: the light distributions are not built for sphere area lights yet");
        if (ql < 0) return fail(RSPT_E_INVALID, "RSPT_QUADRIC_LIGHTS=%s: 0 or 1", getenv("RSPT_QUADRIC_LIGHTS"));
        if (!ql) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere next to a %s: the sphere area light kernels read sphere records only", s->quadric_kinds);
        ql_on = true;
    } else
    if (s->has_sphere_light) {   // served while the sphere-light gate is on (rspt_set_sphere_lights), for a sphere scene the _sl kernels cover; off: today's answer
        const int sl = sphere_lights_mode();
        if (sl < 0) return fail(RSPT_E_INVALID, "RSPT_SPHERE_LIGHTS=%s: 0 or 1", getenv("RSPT_SPHERE_LIGHTS"));
        if (!sl) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere: the light distributions are not built for sphere area lights yet");
        if (s->has_quadrics) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere next to a %s: the sphere area light kernels read sphere records only", s->quadric_kinds);
        if (s->has_maplights) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere next to a %s light: the sphere area light kernels carry no map light", s->maplight_kinds);
    }
    if (ql_on && s->has_maplights) return fail(RSPT_E_UNSUPPORTED, "scene with %s next to a %s light: the quadric area light kernels carry no map light", quadric_scene_lights_what(s), s->maplight_kinds);
    // (a scene with projection / goniometric lights: get_light_dist launches the kernels that carry their arms, and refuses the on-demand table)
    const uint32_t nl = s->dev.n_lights;
    if (nl == 0) return fail(RSPT_E_INVALID, "the scene has no lights");
    HIP_TRY(hipSetDevice(g.device));
    LightDistDev ld;
    const LightDist* lazy = nullptr;
    int rc = get_light_dist(s, strategy, &ld, &lazy);
    if (rc) return rc;
    // SpatialLightDistribution::lookup's voxel addressing (lightdistrib.rs:276-295), as dev_scene.h light_voxel does it
    int32_t pi[3] = {0, 0, 0};
    uint64_t vox = 0;
    if (ld.spatial) {
        for (int i = 0; i < 3; i++) {
            float o = p[i] - s->dev.wb_min[i];
            if (s->dev.wb_max[i] > s->dev.wb_min[i]) o /= s->dev.wb_max[i] - s->dev.wb_min[i];
            const float f = o * (float)ld.nvox[i];
            const int32_t v = (f != f) ? 0 : (f >= 2147483648.0f ? 2147483647 : (f <= -2147483648.0f ? (-2147483647 - 1) : (int32_t)f));
            pi[i] = v < 0 ? 0 : (v > ld.nvox[i] - 1 ? ld.nvox[i] - 1 : v);
        }
        vox = ((uint64_t)pi[2] * ld.nvox[1] + pi[1]) * ld.nvox[0] + pi[0];
    }
    uint64_t row = vox;
    if (lazy) {  // build the voxel if no path has asked for it yet: one round of the on-demand kernels with a one-entry list
        int32_t r = -1;
        HIP_TRY(hipMemcpy(&r, lazy->table + vox, sizeof r, hipMemcpyDeviceToHost));
        if (r < 0) {
            LightLazy lz;
            HIP_TRY(hipMemcpy(&lz, lazy->lazy, sizeof lz, hipMemcpyDeviceToHost));
            if (lz.n_rows >= lz.max_rows) return fail(RSPT_E_NOMEM, "spatial light distribution: row pool exhausted; raise RSPT_LIGHT_TABLE_POOL_BYTES");
            lz.n_new = 1;
            const uint32_t v32 = (uint32_t)vox;
            HIP_TRY(hipMemcpy(lazy->lazy, &lz, sizeof lz, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(lazy->new_list, &v32, sizeof v32, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_ld_contrib_list, dim3(4), dim3(256), 0, g.stream, s->dev, ld.nvox[0], ld.nvox[1], ld.nvox[2], lazy->lazy, lazy->new_list, lazy->func);
            hipLaunchKernelGGL(k_ld_build_list, dim3(1), dim3(64), 0, g.stream, nl, lazy->lazy, lazy->new_list, lazy->func, lazy->cdf, lazy->func_int, lazy->table);
            hipLaunchKernelGGL(k_ld_commit, dim3(1), dim3(1), 0, g.stream, lazy->lazy);
            HIP_TRY(hipStreamSynchronize(g.stream));
            HIP_TRY(hipMemcpy(&r, lazy->table + vox, sizeof r, hipMemcpyDeviceToHost));
        }
        row = (uint64_t)r;
    }
    HIP_TRY(hipMemcpy(func_out, ld.func + row * nl, nl * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cdf_out, ld.cdf + row * (nl + 1), (nl + 1) * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; i++) { if (nvox_out) nvox_out[i] = ld.nvox[i]; if (voxel_out) voxel_out[i] = pi[i]; }
    return RSPT_OK;
}

int rspt_trace_device(rspt_scene_t s, const void* rays_dev, uint64_t n, void* out_dev, int any_hit, int repeat, double* ms_per_launch) {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (!s || (n && (!rays_dev || !out_dev))) return fail(RSPT_E_INVALID, "null argument");
    if (n > 0xfffffff0ull) return fail(RSPT_E_UNSUPPORTED, "more than 2^32 rays per call");
    if (repeat < 1) repeat = 1;
    if (s->has_quadrics && !s->w4_ok) return fail(RSPT_E_UNSUPPORTED, "%s scene with more four-box records than a reference holds", s->quadric_kinds);
    if (s->has_spheres && !s->w4_ok) return fail(RSPT_E_UNSUPPORTED, "sphere scene with more four-box records than a reference holds");
    HIP_TRY(hipSetDevice(g.device));
    if (!g.totals) { int rc = dev_alloc(&g.totals, 8); if (rc) return rc; }
    const bool counters = env_size("RSPT_COUNTERS", 0) != 0;
    if (counters) HIP_TRY(hipMemsetAsync(g.totals, 0, 8 * sizeof(unsigned long long), g.stream));
    hipEvent_t e0 = get_event(0), e1 = get_event(1);
    HIP_TRY(hipEventRecord(e0, g.stream));
    int rc0 = ensure_array(&g.cnt, &g.n_cnt, 4);
    if (!rc0) rc0 = ensure_array(&g.ovf, &g.ovf_cap, std::max<size_t>((size_t)n, 1));
    if (!rc0) rc0 = ensure_spill(pw_spill_threads());
    if (rc0) return rc0;
    TraceCall c; c.count_imm = (uint32_t)n; c.cursor = &g.cnt[0].cursor_closest; c.ra = c.rb = (const rspt_ray*)rays_dev; c.hits = (rspt_hit*)out_dev;
    c.count = counters; c.counters = g.totals; c.xcd_cursors = any_hit ? g.cnt[0].xcd_any : g.cnt[0].xcd_closest;
    for (int r = 0; r < repeat && n; r++) {
        HIP_TRY(hipMemsetAsync(&g.cnt[0], 0, sizeof(QueueCounts), g.stream));
        if (any_hit) launch_trace<true, 1>(trace_grid(), s, c);
        else launch_trace<false, 1>(trace_grid(), s, c);
    }
    HIP_TRY(hipEventRecord(e1, g.stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (ms_per_launch) *ms_per_launch = (double)ms / repeat;
    return RSPT_OK;
}

int rspt_trace(rspt_scene_t s, const rspt_ray* rays, uint64_t n, rspt_hit* out, int any_hit) {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (!s || (n && (!rays || !out))) return fail(RSPT_E_INVALID, "null argument");
    if (n == 0) return RSPT_OK;
    HIP_TRY(hipSetDevice(g.device));
    rspt_ray* rd = nullptr;
    rspt_hit* hd = nullptr;
    HIP_TRY(hipMalloc((void**)&rd, n * sizeof(rspt_ray)));
    hipError_t e = hipMalloc((void**)&hd, n * sizeof(rspt_hit));
    if (e != hipSuccess) { (void)hipFree(rd); return fail(RSPT_E_NOMEM, "%s", hipGetErrorString(e)); }
    int rc = RSPT_OK;
    if (hipMemcpy(rd, rays, n * sizeof(rspt_ray), hipMemcpyHostToDevice) != hipSuccess) rc = fail(RSPT_E_HIP, "upload of rays failed");
    if (!rc) rc = rspt_trace_device(s, rd, n, hd, any_hit, 1, nullptr);
    if (!rc && hipMemcpy(out, hd, n * sizeof(rspt_hit), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(RSPT_E_HIP, "download of hits failed");
    (void)hipFree(rd);
    (void)hipFree(hd);
    return rc;
}

// counters of the last rspt_trace_device / rspt_render when RSPT_COUNTERS=1: out[0] nodes visited, out[1] triangles tested
int rspt_last_counters(uint64_t out[3]) {
    if (!g.inited || !g.totals || !g.cnt) return fail(RSPT_E_INVALID, "no counters");
    unsigned long long t[2];
    HIP_TRY(hipMemcpy(t, g.totals, sizeof t, hipMemcpyDeviceToHost));
    QueueCounts c0;
    HIP_TRY(hipMemcpy(&c0, g.cnt, sizeof c0, hipMemcpyDeviceToHost));
    out[0] = t[0]; out[1] = t[1];
    out[2] = (uint64_t)c0.overflow_closest;  // rspt_trace_device keeps its counters in slot 0
    return RSPT_OK;
}

int rspt_dev_alloc(uint64_t bytes, void** out) {
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (!out) return fail(RSPT_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(g.device));
    HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
    return RSPT_OK;
}
int rspt_dev_free(void* p) {
    if (p) HIP_TRY(hipFree(p));
    return RSPT_OK;
}
int rspt_dev_upload(void* dst, const void* src, uint64_t bytes) {
    if (bytes && (!dst || !src)) return fail(RSPT_E_INVALID, "null argument");
    if (bytes) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return RSPT_OK;
}
int rspt_dev_download(void* dst, const void* src, uint64_t bytes) {
    if (bytes && (!dst || !src)) return fail(RSPT_E_INVALID, "null argument");
    if (bytes) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RSPT_OK;
}

}  // extern "C"
