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
#include <functional>
#include <limits>
#include <map>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rspt.h"
#include "material_assembly.h"
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
    std::vector<void*> allocs;
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
    bool has_sphere_light = false;    // an emissive sphere: refused by rspt_render and the light-distribution hook (sphere area lights are not on the device)
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

// Light distribution for (scene, strategy): create_light_sample_distribution (lightdistrib.rs:393-418)
int get_light_dist(rspt_scene_s* s, uint32_t strategy, LightDistDev* out, const LightDist** lazy_out = nullptr) {
    const uint32_t nl = s->dev.n_lights;
    *out = LightDistDev{};
    out->nvox[0] = out->nvox[1] = out->nvox[2] = 1;
    if (nl == 0) return RSPT_OK;
    int eff = (strategy == RSPT_LIGHTS_UNIFORM || nl == 1) ? RSPT_LIGHTS_UNIFORM : (strategy == RSPT_LIGHTS_POWER ? RSPT_LIGHTS_POWER : RSPT_LIGHTS_SPATIAL);
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
            hipLaunchKernelGGL(s->has_maplights ? k_ld_contrib_ml : k_ld_contrib, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, g.stream, s->dev, d.nvox[0], d.nvox[1], d.nvox[2], d.func);
            hipLaunchKernelGGL(k_ld_build, dim3((uint32_t)((n_vox + 255) / 256)), dim3(256), 0, g.stream, (uint32_t)n_vox, nl, 0, d.func, d.cdf, d.func_int);
        } else {
            hipLaunchKernelGGL(s->has_maplights ? k_ld_fixed_ml : k_ld_fixed, dim3((nl + 255) / 256), dim3(256), 0, g.stream, s->dev, eff == RSPT_LIGHTS_POWER ? 1 : 0, d.func);
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

}  // namespace

extern "C" {

int rspt_abi_version(void) { return RSPT_ABI_VERSION; }
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
    if (!g.inited) return fail(RSPT_E_NODEVICE, "rspt_init has not been called");
    if (!d || !out) return fail(RSPT_E_INVALID, "null argument");
    *out = nullptr;
    if (d->n_prims > 0x7fffffffull || d->n_nodes > 0x7fffffffull) return fail(RSPT_E_UNSUPPORTED, "more than 2^31 primitives / nodes");
    if ((d->n_nodes && !d->nodes) || (d->n_prims && (!d->prims || !d->meshes || !d->P)) || (d->n_materials && !d->materials) ||
        (d->n_lights && !d->lights))
        return fail(RSPT_E_INVALID, "null array with non-zero count");
    if ((d->n_nodes == 0) != (d->n_prims == 0)) return fail(RSPT_E_INVALID, "nodes and prims must both be empty or both non-empty");
    // ---- validate indices on the host (a bad scene must not fault the GPU) ----
    bool has_null = false;
    const bool instanced = d->n_instances > 0;
    const uint64_t n_top_prims = instanced ? d->n_top_prims : d->n_prims, n_top_nodes = instanced ? d->n_top_nodes : d->n_nodes;
    if (d->n_spheres && instanced) return fail(RSPT_E_UNSUPPORTED, "spheres together with object instances");   // (ABI 23: a follow-up)
    if (d->n_disks && instanced) return fail(RSPT_E_UNSUPPORTED, "disks together with object instances");
    if (d->n_cylinders && instanced) return fail(RSPT_E_UNSUPPORTED, "cylinders together with object instances");
    if (instanced) {  // objects + instances behind the top-level aggregate
        if (!d->instances || !d->objects || d->n_objects == 0) return fail(RSPT_E_INVALID, "instances without objects");
        if (n_top_prims > d->n_prims || n_top_nodes > d->n_nodes || n_top_nodes == 0) return fail(RSPT_E_INVALID, "bad top-level aggregate range");
        if (d->instancing_mode != RSPT_INSTANCING_REFERENCE && d->instancing_mode != RSPT_INSTANCING_FIXED) return fail(RSPT_E_INVALID, "bad instancing_mode");
        for (uint32_t i = 0; i < d->n_objects; i++) {
            const rspt_object& o = d->objects[i];
            if (o.n_prims == 0 || o.first_prim < n_top_prims || o.first_prim + o.n_prims > d->n_prims) return fail(RSPT_E_INVALID, "object %u: primitive range", i);
            if (o.n_nodes == 0 ? o.n_prims != 1 : (o.first_node < n_top_nodes || o.first_node + o.n_nodes > d->n_nodes)) return fail(RSPT_E_INVALID, "object %u: node range", i);
        }
        for (uint32_t i = 0; i < d->n_instances; i++) {
            const rspt_instance& in = d->instances[i];
            if (in.object >= d->n_objects) return fail(RSPT_E_INVALID, "instance %u: object index out of range", i);
            for (int k = 0; k < 2; k++) {   // (rows 3 other than (0 0 0 1) are served: InstDev::m3 / mi3; a weight of 0 is where the reference asserts, transform.rs:747)
                const float* m = k ? in.from_world : in.to_world;
                if (!std::isfinite(m[12]) || !std::isfinite(m[13]) || !std::isfinite(m[14]) || !std::isfinite(m[15])) return fail(RSPT_E_INVALID, "instance %u: non-finite transform", i);
                for (int j = 0; j < 12; j++) if (!(fabsf(m[j]) < RSPT_INF)) return fail(RSPT_E_INVALID, "instance %u: non-finite transform", i);
            }
        }
    }
    // ABI 23: spheres (dev_sphere.h)
    if (d->n_spheres && !d->spheres) return fail(RSPT_E_INVALID, "null spheres with n_spheres > 0");
    for (uint32_t i = 0; i < d->n_spheres; i++) {
        const rspt_sphere& sp = d->spheres[i];
        for (int k = 0; k < 16; k++)
            if (!std::isfinite(sp.object_to_world[k]) || !std::isfinite(sp.world_to_object[k])) return fail(RSPT_E_INVALID, "sphere %u: non-finite transform", i);
        if (!(sp.radius > 0.0f) || !std::isfinite(sp.radius) || !std::isfinite(sp.z_min) || !std::isfinite(sp.z_max) || !std::isfinite(sp.phi_max) ||
            !std::isfinite(sp.theta_min) || !std::isfinite(sp.theta_max))
            return fail(RSPT_E_INVALID, "sphere %u: radius must be positive and finite, z / theta / phi finite", i);
        if (sp.medium_inside > d->n_media || sp.medium_outside > d->n_media) return fail(RSPT_E_INVALID, "sphere %u: medium index out of range", i);
    }
    // ABI 27: disks and cylinders (dev_quadric.h)
    if (d->n_disks && !d->disks) return fail(RSPT_E_INVALID, "null disks with n_disks > 0");
    if (d->n_cylinders && !d->cylinders) return fail(RSPT_E_INVALID, "null cylinders with n_cylinders > 0");
    if ((uint64_t)d->n_spheres + d->n_disks + d->n_cylinders > 0x7fffffffull) return fail(RSPT_E_UNSUPPORTED, "more than 2^31 spheres, disks and cylinders");
    for (uint32_t i = 0; i < d->n_disks; i++) {
        const rspt_disk& k = d->disks[i];
        for (int j = 0; j < 16; j++)
            if (!std::isfinite(k.object_to_world[j]) || !std::isfinite(k.world_to_object[j])) return fail(RSPT_E_INVALID, "disk %u: non-finite transform", i);
        if (!std::isfinite(k.height) || !std::isfinite(k.radius) || !std::isfinite(k.inner_radius) || !std::isfinite(k.phi_max)) return fail(RSPT_E_INVALID, "disk %u: non-finite parameter", i);
        if (!(k.radius > 0.0f)) return fail(RSPT_E_INVALID, "disk %u: radius must be positive", i);
        if (k.radius == k.inner_radius) return fail(RSPT_E_INVALID, "disk %u: radius equals inner_radius (v divides by their difference)", i);
        if (!(k.phi_max > 0.0f && k.phi_max <= 2.0f * RSPT_PI)) return fail(RSPT_E_INVALID, "disk %u: phi_max outside (0, 2 pi]", i);
        if (k.medium_inside > d->n_media || k.medium_outside > d->n_media) return fail(RSPT_E_INVALID, "disk %u: medium index out of range", i);
    }
    for (uint32_t i = 0; i < d->n_cylinders; i++) {
        const rspt_cylinder& k = d->cylinders[i];
        for (int j = 0; j < 16; j++)
            if (!std::isfinite(k.object_to_world[j]) || !std::isfinite(k.world_to_object[j])) return fail(RSPT_E_INVALID, "cylinder %u: non-finite transform", i);
        if (!std::isfinite(k.radius) || !std::isfinite(k.z_min) || !std::isfinite(k.z_max) || !std::isfinite(k.phi_max)) return fail(RSPT_E_INVALID, "cylinder %u: non-finite parameter", i);
        if (!(k.radius > 0.0f)) return fail(RSPT_E_INVALID, "cylinder %u: radius must be positive", i);
        if (k.z_min == k.z_max) return fail(RSPT_E_INVALID, "cylinder %u: z_min equals z_max (v divides by their difference)", i);
        if (!(k.phi_max > 0.0f && k.phi_max <= 2.0f * RSPT_PI)) return fail(RSPT_E_INVALID, "cylinder %u: phi_max outside (0, 2 pi]", i);
        if (k.medium_inside > d->n_media || k.medium_outside > d->n_media) return fail(RSPT_E_INVALID, "cylinder %u: medium index out of range", i);
    }
    bool disk_light = false, cylinder_light = false;
    for (uint64_t i = 0; i < d->n_prims; i++) {
        const rspt_prim& p = d->prims[i];
        if (p.mesh == RSPT_MESH_DISK || p.mesh == RSPT_MESH_CYLINDER) {
            const bool dk = p.mesh == RSPT_MESH_DISK;
            const char* kn = dk ? "disk" : "cylinder";
            if (p.v[0] >= (dk ? d->n_disks : d->n_cylinders)) return fail(RSPT_E_INVALID, "prim %llu: %s index out of range", (unsigned long long)i, kn);
            if (p.material != 0xffffffffu && p.material >= d->n_materials) return fail(RSPT_E_INVALID, "prim %llu: %s's material index out of range", (unsigned long long)i, kn);
            if (p.area_light < -1 || p.area_light >= (int64_t)d->n_lights) return fail(RSPT_E_INVALID, "prim %llu: %s's light index out of range", (unsigned long long)i, kn);
            if (p.area_light >= 0 && (d->lights[p.area_light].kind != RSPT_LIGHT_DIFFUSE_AREA || d->lights[p.area_light].prim != i))
                return fail(RSPT_E_INVALID, "prim %llu: %s's area light %d is not a DIFFUSE_AREA light on this primitive", (unsigned long long)i, kn, p.area_light);
            if (p.area_light >= 0) (dk ? disk_light : cylinder_light) = true;
            has_null |= p.material == 0xffffffffu;
            continue;
        }
        if (p.mesh == RSPT_MESH_SPHERE) {
            if (p.v[0] >= d->n_spheres) return fail(RSPT_E_INVALID, "prim %llu: sphere index out of range", (unsigned long long)i);
            if (p.material != 0xffffffffu && p.material >= d->n_materials) return fail(RSPT_E_INVALID, "prim %llu: material index out of range", (unsigned long long)i);
            if (p.area_light < -1 || p.area_light >= (int64_t)d->n_lights) return fail(RSPT_E_INVALID, "prim %llu: sphere's light index out of range", (unsigned long long)i);
            // an emissive sphere: its light is a DiffuseAreaLight on this very primitive (the pairing api.rs makes, and rspt_light.prim states)
            if (p.area_light >= 0 && (d->lights[p.area_light].kind != RSPT_LIGHT_DIFFUSE_AREA || d->lights[p.area_light].prim != i))
                return fail(RSPT_E_INVALID, "prim %llu: sphere's area light %d is not a DIFFUSE_AREA light on this primitive", (unsigned long long)i, p.area_light);
            has_null |= p.material == 0xffffffffu;
            continue;
        }
        if (p.mesh == RSPT_MESH_INSTANCE) {
            if (!instanced || i >= n_top_prims || p.v[0] >= d->n_instances) return fail(RSPT_E_INVALID, "prim %llu: bad instance reference", (unsigned long long)i);
            continue;
        }
        if (i >= n_top_prims && p.area_light != -1) return fail(RSPT_E_UNSUPPORTED, "prim %llu: area lights are not supported with object instancing (api.rs:2899)", (unsigned long long)i);
        if (p.v[0] >= d->n_vertices || p.v[1] >= d->n_vertices || p.v[2] >= d->n_vertices) return fail(RSPT_E_INVALID, "prim %llu: vertex index out of range", (unsigned long long)i);
        if (p.mesh >= d->n_meshes) return fail(RSPT_E_INVALID, "prim %llu: mesh index out of range", (unsigned long long)i);
        if (p.material != 0xffffffffu && p.material >= d->n_materials) return fail(RSPT_E_INVALID, "prim %llu: material index out of range", (unsigned long long)i);
        if (p.area_light >= (int64_t)d->n_lights) return fail(RSPT_E_INVALID, "prim %llu: light index out of range", (unsigned long long)i);
        has_null |= p.material == 0xffffffffu;
    }
    bool any_alpha = false;
    for (uint32_t i = 0; i < d->n_meshes; i++) {
        const rspt_mesh& m = d->meshes[i];
        if (m.alpha_tex > d->n_textures || m.shadow_alpha_tex > d->n_textures) return fail(RSPT_E_INVALID, "mesh %u: alpha texture index out of range", i);
        any_alpha |= m.alpha_tex != 0 || m.shadow_alpha_tex != 0;
        if (m.medium_inside > d->n_media || m.medium_outside > d->n_media) return fail(RSPT_E_INVALID, "mesh %u: medium index out of range", i);
    }
    if (d->n_media && !d->media) return fail(RSPT_E_INVALID, "null media");
    for (uint32_t i = 0; i < d->n_media; i++) {
        const rspt_medium& m = d->media[i];
        if (m.kind != RSPT_MEDIUM_HOMOGENEOUS && m.kind != RSPT_MEDIUM_GRID) return fail(RSPT_E_UNSUPPORTED, "medium %u: kind %u (homogeneous and grid-density media)", i, m.kind);
        if (m.kind == RSPT_MEDIUM_GRID) {
            if (m.nx < 1 || m.ny < 1 || m.nz < 1 || (uint64_t)m.nx * m.ny * m.nz > (1ull << 31) || !m.density) return fail(RSPT_E_INVALID, "medium %u: bad density grid", i);
            const float* w = m.world_to_medium;
            if (w[12] != 0.0f || w[13] != 0.0f || w[14] != 0.0f || w[15] != 1.0f) return fail(RSPT_E_UNSUPPORTED, "medium %u: projective world_to_medium", i);
        }
        for (int c = 0; c < 3; c++)
            if (!(m.sigma_a[c] >= 0.0f) || !(m.sigma_s[c] >= 0.0f) || !std::isfinite(m.sigma_a[c]) || !std::isfinite(m.sigma_s[c])) return fail(RSPT_E_INVALID, "medium %u: bad sigma_a / sigma_s", i);
        if (!(m.g > -1.0f && m.g < 1.0f)) return fail(RSPT_E_INVALID, "medium %u: g outside (-1, 1)", i);
    }
    if (any_alpha)
        for (uint64_t i = 0; i < d->n_prims; i++) {
            const rspt_prim& p = d->prims[i];
            if (p.mesh < d->n_meshes && p.area_light >= 0 && (d->meshes[p.mesh].alpha_tex || d->meshes[p.mesh].shadow_alpha_tex))
                return fail(RSPT_E_UNSUPPORTED, "prim %llu: an emissive mesh with an alpha mask", (unsigned long long)i);
        }
    bool has_maplights = false, has_projection = false, has_goniometric = false;
    for (uint32_t i = 0; i < d->n_lights; i++) {
        if (d->lights[i].kind < RSPT_LIGHT_DIFFUSE_AREA || d->lights[i].kind > RSPT_LIGHT_GONIOMETRIC) return fail(RSPT_E_UNSUPPORTED, "light %u: unsupported kind %u", i, d->lights[i].kind);
        if (d->lights[i].kind == RSPT_LIGHT_DIFFUSE_AREA && (d->lights[i].prim >= n_top_prims || d->prims[d->lights[i].prim].mesh == RSPT_MESH_INSTANCE))   // (a sphere primitive may be named, ABI 23)
            return fail(RSPT_E_INVALID, "light %u: prim out of range", i);
        if (d->lights[i].kind == RSPT_LIGHT_DIFFUSE_AREA && d->prims[d->lights[i].prim].mesh == RSPT_MESH_SPHERE && d->prims[d->lights[i].prim].area_light != (int32_t)i)
            return fail(RSPT_E_INVALID, "light %u: its sphere primitive names another light", i);
        if (d->lights[i].kind == RSPT_LIGHT_DIFFUSE_AREA && (d->prims[d->lights[i].prim].mesh == RSPT_MESH_DISK || d->prims[d->lights[i].prim].mesh == RSPT_MESH_CYLINDER) &&
            d->prims[d->lights[i].prim].area_light != (int32_t)i)
            return fail(RSPT_E_INVALID, "light %u: its %s primitive names another light", i, d->prims[d->lights[i].prim].mesh == RSPT_MESH_DISK ? "disk" : "cylinder");
        if (d->lights[i].kind == RSPT_LIGHT_INFINITE && d->lights[i].prim >= d->n_envmaps) return fail(RSPT_E_INVALID, "light %u: envmap index out of range", i);
        if (d->lights[i].kind == RSPT_LIGHT_PROJECTION || d->lights[i].kind == RSPT_LIGHT_GONIOMETRIC) {   // ABI 24
            const rspt_light& l = d->lights[i];
            const char* kn = l.kind == RSPT_LIGHT_PROJECTION ? "projection" : "goniometric";
            const int n_par = l.kind == RSPT_LIGHT_PROJECTION ? 22 : 12;
            for (int k = 0; k < 3; k++) if (!std::isfinite(l.L[k])) return fail(RSPT_E_INVALID, "light %u (%s): non-finite intensity", i, kn);
            for (int k = 0; k < n_par; k++) if (!std::isfinite(l.p[k])) return fail(RSPT_E_INVALID, "light %u (%s): non-finite parameter p[%d]", i, kn, k);
            if (l.prim != 0xffffffffu && l.prim >= d->n_envmaps) return fail(RSPT_E_INVALID, "light %u (%s): map index out of range", i, kn);
            if (l.kind == RSPT_LIGHT_PROJECTION && (l.p[12] > l.p[14] || l.p[13] > l.p[15])) return fail(RSPT_E_INVALID, "light %u (projection): screen_bounds min above max", i);
            has_maplights = true;
            (l.kind == RSPT_LIGHT_PROJECTION ? has_projection : has_goniometric) = true;
        }
    }
    // textures: constant / imagemap / scale; each material may bind at most RSPT_TEX_SLOTS distinct ones
    if ((d->n_textures && !d->textures) || (d->n_images && !d->images)) return fail(RSPT_E_INVALID, "null texture / image array");
    for (uint32_t i = 0; i < d->n_images; i++) {
        const rspt_image& im = d->images[i];
        auto pow2 = [](uint32_t v) { return v && !(v & (v - 1)); };
        if (!pow2(im.width) || !pow2(im.height) || im.width > 32768 || im.height > 32768) return fail(RSPT_E_INVALID, "image %u: sides must be powers of two <= 32768 (MipMap::new resamples first)", i);
        uint32_t nl = 1;
        for (uint32_t m = std::max(im.width, im.height); m > 1; m >>= 1) nl++;
        if (im.n_levels != nl || nl > 16) return fail(RSPT_E_INVALID, "image %u: n_levels %u, expected %u", i, im.n_levels, nl);
        if (!im.texels || (im.channels != 1 && im.channels != 3)) return fail(RSPT_E_INVALID, "image %u: null texels or channels not 1 / 3", i);
    }
    {   // texture graph: kinds, mappings, child indices, depth (dev_texture.h evaluates at most RSPT_TEX_MAX_DEPTH levels)
        std::vector<int> depth(d->n_textures, 0);  // 0 = not computed, -1 = on the current path (cycle)
        std::function<int(uint32_t)> depth_of = [&](uint32_t i) -> int {
            if (depth[i] > 0) return depth[i];
            if (depth[i] < 0) return 1000;
            depth[i] = -1;
            const rspt_texture& t = d->textures[i];
            int dmax = 0;
            const uint32_t kids[3] = {t.tex1, t.tex2, t.tex3};
            const int n_kids = t.kind == RSPT_TEX_MIX ? 3 : ((t.kind == RSPT_TEX_SCALE || t.kind == RSPT_TEX_CHECKERBOARD || t.kind == RSPT_TEX_DOTS) ? 2 : 0);
            for (int k = 0; k < n_kids; k++) dmax = std::max(dmax, kids[k] < d->n_textures ? depth_of(kids[k]) : 1000);
            return depth[i] = 1 + dmax;
        };
        for (uint32_t i = 0; i < d->n_textures; i++) {
            const rspt_texture& t = d->textures[i];
            if (t.kind < RSPT_TEX_CONSTANT || t.kind > RSPT_TEX_WRINKLED) return fail(RSPT_E_UNSUPPORTED, "texture %u: unsupported kind %u", i, t.kind);
            const bool map2d = t.kind == RSPT_TEX_IMAGE || t.kind == RSPT_TEX_CHECKERBOARD || t.kind == RSPT_TEX_DOTS;
            const bool map3d = t.kind == RSPT_TEX_FBM || t.kind == RSPT_TEX_MARBLE || t.kind == RSPT_TEX_WINDY || t.kind == RSPT_TEX_WRINKLED;
            if (map2d && (t.mapping < RSPT_MAP_UV || t.mapping > RSPT_MAP_CYLINDRICAL)) return fail(RSPT_E_UNSUPPORTED, "texture %u: 2-D mapping %u", i, t.mapping);
            if (map3d && t.mapping != RSPT_MAP_IDENTITY3D) return fail(RSPT_E_UNSUPPORTED, "texture %u: 3-D textures take the identity mapping", i);
            if (map3d && (t.octaves < 0 || t.octaves > 64)) return fail(RSPT_E_INVALID, "texture %u: octaves out of range", i);
            if (t.kind == RSPT_TEX_IMAGE) {
                if (t.image >= d->n_images) return fail(RSPT_E_INVALID, "texture %u: image index out of range", i);
                if (t.wrap > RSPT_WRAP_CLAMP) return fail(RSPT_E_INVALID, "texture %u: bad wrap mode", i);
            }
            const int dep = depth_of(i);
            if (dep >= 1000) return fail(RSPT_E_INVALID, "texture %u: child index out of range or cyclic graph", i);
            if (dep > RSPT_TEX_MAX_DEPTH) return fail(RSPT_E_UNSUPPORTED, "texture %u: graph deeper than %d levels", i, RSPT_TEX_MAX_DEPTH);
        }
    }
    // materials: Material::compute_scattering_functions restated on the host (material_assembly.h), once per allow_multiple_lobes
    std::vector<rspt_material> asm_mats[2];
    std::vector<rspt_bxdf> asm_bx[2];
    std::vector<rspt_mat::DynMaterial> asm_dyn[2];   // [material] when the variant has a dynamic material, else empty
    std::vector<uint8_t> asm_is_dyn[2];
    for (int v = 0; v < 2; v++) {
        rspt_mat::Assembler as(d, v == 0);
        rspt_mat::Lobes lb;
        asm_mats[v].resize(d->n_materials);
        asm_is_dyn[v].assign(d->n_materials, 0);
        for (uint32_t i = 0; i < d->n_materials; i++) {
            if (rspt_mat::Error e = as.assemble(i, &lb)) return fail(e.code, "%s", e.text.c_str());
            lb.mat.first_bxdf = (uint32_t)asm_bx[v].size();
            asm_mats[v][i] = lb.mat;
            asm_bx[v].insert(asm_bx[v].end(), lb.lobes.begin(), lb.lobes.end());
            if (lb.dynamic) {
                if (asm_dyn[v].empty()) asm_dyn[v].resize(d->n_materials);
                asm_dyn[v][i] = lb.dyn;
                asm_is_dyn[v][i] = 1;
            }
        }
    }
    uint32_t shade_features = 0;
    for (int v = 0; v < 2; v++)
        for (const rspt_bxdf& b : asm_bx[v]) {
            shade_features |= RSPT_SF_LOBE(b.type);
            if (b.fresnel == RSPT_FRESNEL_CONDUCTOR) shade_features |= SF_CONDUCTOR;
            if (b.has_sc) shade_features |= SF_SC;
            if (b.tex_r || b.tex_t || b.tex_ax || b.tex_ay) shade_features |= SF_TEX;
        }
    for (int v = 0; v < 2; v++)
        for (const rspt_material& m : asm_mats[v]) if (m.bump_tex) shade_features |= SF_TEX;
    uint32_t shade_classes = 0;
    {   // materials whose lobe lists have the same types in the same order (and the same textured-ness) cost a wave the same
        std::vector<std::string> seen;
        for (uint32_t i = 0; i < d->n_materials; i++) {
            const rspt_material& m = asm_mats[0][i];
            std::string sig = asm_is_dyn[0][i] ? "dyn" : "";
            for (uint32_t l = 0; l < m.n_bxdfs; l++) {
                const rspt_bxdf& b = asm_bx[0][m.first_bxdf + l];
                sig += (char)('a' + b.type); sig += (char)('0' + b.fresnel); sig += (b.tex_r || b.tex_t || b.tex_ax || b.tex_ay) ? 't' : 'c';
            }
            if (m.bump_tex) sig += 'B';
            if (std::find(seen.begin(), seen.end(), sig) == seen.end()) seen.push_back(sig);
        }
        shade_classes = (uint32_t)seen.size();
    }
    if (!asm_dyn[0].empty() || !asm_dyn[1].empty())  // a list built per hit may hold any lobe its material kind can push
        shade_features |= SF_DYNAMIC | SF_TEX | 0x3feu | SF_CONDUCTOR | SF_SC;
    for (uint32_t i = 0; i < d->n_lights; i++) {
        const uint32_t k = d->lights[i].kind;
        shade_features |= k == RSPT_LIGHT_DIFFUSE_AREA ? SF_L_AREA : (k == RSPT_LIGHT_POINT ? SF_L_POINT : (k == RSPT_LIGHT_SPOT ? SF_L_SPOT : (k == RSPT_LIGHT_DISTANT ? SF_L_DISTANT : (k == RSPT_LIGHT_INFINITE ? SF_L_INFINITE : SF_L_MAP))));
    }
    for (uint32_t i = 0; i < d->n_meshes; i++)
        if (d->meshes[i].has_n || d->meshes[i].has_s || d->meshes[i].has_uv) shade_features |= SF_VERTEX;
    if (instanced) shade_features |= SF_INST;
    if (has_null || (instanced && d->instancing_mode == RSPT_INSTANCING_REFERENCE)) shade_features |= SF_NULL;
    if (d->n_envmaps && !d->envmaps) return fail(RSPT_E_INVALID, "null envmaps");
    for (uint32_t i = 0; i < d->n_envmaps; i++) {
        const rspt_envmap& e = d->envmaps[i];
        auto pow2 = [](uint32_t v) { return v && !(v & (v - 1)); };
        if (!pow2(e.width) || !pow2(e.height) || e.width > 32768 || e.height > 32768) return fail(RSPT_E_INVALID, "envmap %u: sides must be powers of two <= 32768", i);
        uint32_t nl = 1;
        for (uint32_t m = std::max(e.width, e.height); m > 1; m >>= 1) nl++;
        if (e.n_levels != nl || nl > 16) return fail(RSPT_E_INVALID, "envmap %u: n_levels %u, expected %u", i, e.n_levels, nl);
        // ABI 24: a map that only projection / goniometric lights name carries no distribution (they never sample it); an infinite light needs its own
        bool sampled = false, named = false;
        for (uint32_t l = 0; l < d->n_lights; l++) {
            if (d->lights[l].kind == RSPT_LIGHT_INFINITE && d->lights[l].prim == i) sampled = true;
            if ((d->lights[l].kind == RSPT_LIGHT_PROJECTION || d->lights[l].kind == RSPT_LIGHT_GONIOMETRIC) && d->lights[l].prim == i) named = true;
        }
        const bool no_dist = !e.dist_func && e.dist_nu == 0 && e.dist_nv == 0;
        if (!e.texels || !((named && !sampled && no_dist) || (e.dist_func && e.dist_nu != 0 && e.dist_nv != 0))) return fail(RSPT_E_INVALID, "envmap %u: null data", i);
    }
    // BVH: child / leaf ranges in bounds, depth <= 64 (the reference's fixed traversal stack, bvh.rs:420); with instances the
    // object's traversal continues on the stack of the top-level one (kernels.h traverse), so the two depths add up
    {
        std::string err;
        auto tree_depth = [&](uint64_t root, uint64_t node_lo, uint64_t node_hi, uint64_t prim_lo, uint64_t prim_hi) -> int {
            std::vector<std::pair<uint32_t, uint32_t>> stack;  // node, depth
            stack.push_back({(uint32_t)root, 1u});
            uint64_t visited = 0;
            uint32_t deepest = 0;
            while (!stack.empty()) {
                auto [ni, depth] = stack.back();
                stack.pop_back();
                if (++visited > node_hi - node_lo) { err = "BVH is not a tree"; return -1; }
                deepest = std::max(deepest, depth);
                if (depth > 64) { err = "BVH deeper than the 64-entry traversal stack"; return -2; }
                const rspt_bvh_node& n = d->nodes[ni];
                if (n.n_prims > 0) {
                    if (n.offset < 0 || (uint64_t)n.offset < prim_lo || (uint64_t)n.offset + n.n_prims > prim_hi) { err = "node " + std::to_string(ni) + ": leaf range out of bounds"; return -1; }
                } else {
                    if (n.axis > 2 || n.offset <= (int64_t)ni || (uint64_t)n.offset >= node_hi || (uint64_t)ni + 1 >= node_hi) { err = "node " + std::to_string(ni) + ": bad children"; return -1; }
                    stack.push_back({(uint32_t)n.offset, depth + 1});
                    stack.push_back({ni + 1, depth + 1});
                }
            }
            return (int)deepest;
        };
        int top_depth = 0, obj_depth = 0;
        if (d->n_nodes) {
            top_depth = tree_depth(0, 0, n_top_nodes, 0, n_top_prims);
            if (top_depth < 0) return fail(top_depth == -2 ? RSPT_E_UNSUPPORTED : RSPT_E_INVALID, "%s", err.c_str());
        }
        for (uint32_t i = 0; instanced && i < d->n_objects; i++) {
            const rspt_object& o = d->objects[i];
            if (o.n_nodes == 0) continue;
            const int dep = tree_depth(o.first_node, o.first_node, o.first_node + o.n_nodes, o.first_prim, o.first_prim + o.n_prims);
            if (dep < 0) return fail(dep == -2 ? RSPT_E_UNSUPPORTED : RSPT_E_INVALID, "object %u: %s", i, err.c_str());
            obj_depth = std::max(obj_depth, dep);
        }
        if (top_depth + obj_depth > 64) return fail(RSPT_E_UNSUPPORTED, "top-level BVH (%d levels) + object BVH (%d levels) deeper than the 64-entry traversal stack", top_depth, obj_depth);
    }
    HIP_TRY(hipSetDevice(g.device));
    rspt_scene_s* s = new rspt_scene_s();
    s->dev.time_div = 1u;
    s->has_null_material = has_null || (instanced && d->instancing_mode == RSPT_INSTANCING_REFERENCE);  // instanced hits pass through like null surfaces (Q11)
    s->has_instances = instanced;
    s->has_alpha = any_alpha;
    s->has_maplights = has_maplights;
    s->maplight_kinds = has_projection ? (has_goniometric ? "projection and goniometric" : "projection") : (has_goniometric ? "goniometric" : "");
    s->n_materials = d->n_materials;
    s->shade_features = shade_features;
    s->shade_classes = shade_classes;
    auto bail = [&](int rc) {
        for (void* p : s->allocs) (void)hipFree(p);
        delete s;
        return rc;
    };
    int rc;
    const rspt_bvh_node* nodes_d = nullptr;
    const rspt_mesh* meshes_d = nullptr;
    const float* P_d = nullptr;
    if ((rc = upload(s, d->nodes, d->n_nodes, &nodes_d))) return bail(rc);
    const bool quadrics = d->n_disks || d->n_cylinders;
    if (quadrics) {   // ABI 27: on the device a disk or cylinder primitive is a sphere primitive whose index names its slot behind the triangle records (dev_quadric.h: spheres, disks, cylinders)
        std::vector<rspt_prim> pv(d->prims, d->prims + d->n_prims);
        for (rspt_prim& p : pv) {
            if (p.mesh == RSPT_MESH_DISK) { p.mesh = RSPT_MESH_SPHERE; p.v[0] += d->n_spheres; }
            else if (p.mesh == RSPT_MESH_CYLINDER) { p.mesh = RSPT_MESH_SPHERE; p.v[0] += d->n_spheres + d->n_disks; }
        }
        if ((rc = upload(s, pv.data(), pv.size(), &s->dev.prims))) return bail(rc);
    } else
    if ((rc = upload(s, d->prims, d->n_prims, &s->dev.prims))) return bail(rc);
    if ((rc = upload(s, d->meshes, d->n_meshes, &meshes_d))) return bail(rc);
    s->dev.meshes = meshes_d;
    {   // media: a grid medium's density goes to the device, its record gets the device pointer and 1 / max(density) (GridDensityMedium::new, grid.rs:44-55)
        std::vector<rspt_medium> media(d->media, d->media + d->n_media);
        for (rspt_medium& m : media) {
            if (m.kind != RSPT_MEDIUM_GRID) continue;
            const size_t n = (size_t)m.nx * m.ny * m.nz;
            float max_density = 0.0f;
            for (size_t k = 0; k < n; k++) max_density = std::fmax(max_density, m.density[k]);   // f32::max
            const float inv_max = 1.0f / max_density;
            memcpy(&m.pad, &inv_max, sizeof inv_max);
            const float* dens_d = nullptr;
            if ((rc = upload(s, m.density, n, &dens_d))) return bail(rc);
            m.density = dens_d;
            s->dev.n_grid_media++;
        }
        if ((rc = upload(s, media.data(), media.size(), &s->dev.media))) return bail(rc);
    }
    s->dev.n_media = d->n_media;
    if ((rc = upload(s, d->P, d->n_vertices * 3, &P_d))) return bail(rc);
    if ((rc = upload(s, d->N, d->N ? d->n_vertices * 3 : 0, &s->dev.N))) return bail(rc);
    if ((rc = upload(s, d->S, d->S ? d->n_vertices * 3 : 0, &s->dev.S))) return bail(rc);
    if ((rc = upload(s, d->UV, d->UV ? d->n_vertices * 2 : 0, &s->dev.UV))) return bail(rc);
    {   // SceneDev::tri_nuv: every primitive's normals and uvs next to each other (80 B per primitive; skipped beyond 16 GB)
        bool any = false;
        for (uint32_t i = 0; i < d->n_meshes; i++) any = any || (d->meshes[i].has_n && d->N) || (d->meshes[i].has_uv && d->UV);
        if (any && d->n_prims && d->n_prims * 80ull <= env_size("RSPT_TRI_NUV_MAX_BYTES", (size_t)16 << 30) && env_size("RSPT_TRI_NUV", 1) != 0) {
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
            const float* dev_nuv = nullptr;
            if ((rc = upload(s, nuv.data(), nuv.size(), &dev_nuv))) return bail(rc);
            s->dev.tri_nuv = reinterpret_cast<const float4*>(dev_nuv);
        }
    }
    {   // lobes: texture ids become per-material slot numbers (1 + slot) for k_texture / k_shade
        bool any = false;
        for (int v = 0; v < 2; v++) {
            std::vector<rspt_bxdf>& bx = asm_bx[v];
            std::vector<uint32_t> slots((size_t)d->n_materials * RSPT_TEX_SLOTS, 0xffffffffu);
            std::vector<uint8_t> mflags(d->n_materials, 0);
            bool any_v = false;
            for (uint32_t m = 0; m < d->n_materials; m++) {
                const rspt_material& mat = asm_mats[v][m];
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
                if (full) return bail(fail(RSPT_E_UNSUPPORTED, "material %u binds more than %d distinct textures", m, RSPT_TEX_SLOTS));
                if (asm_is_dyn[v][m]) mflags[m] |= RSPT_MAT_DYNAMIC | RSPT_MAT_TEXTURED;
                if (mat.bump_tex) mflags[m] |= RSPT_MAT_BUMP;
                any_v |= mflags[m] != 0;
            }
            rspt_scene_s::MatSet& ms = s->mat_set[v];
            ms.textured = any_v;
            ms.dynamic = !asm_dyn[v].empty();
            if (ms.dynamic && (rc = upload(s, asm_dyn[v].data(), asm_dyn[v].size(), &ms.dyn))) return bail(rc);
            any |= any_v;
            if ((rc = upload(s, asm_mats[v].data(), asm_mats[v].size(), &ms.materials)) || (rc = upload(s, bx.data(), bx.size(), &ms.bxdfs)) ||
                (rc = upload(s, slots.data(), slots.size(), &ms.mat_slots)) || (rc = upload(s, mflags.data(), mflags.size(), &ms.mat_flags)))
                return bail(rc);
        }
        s->select_materials(true);
        if (any || any_alpha) {  // k_texture / per-path texture rows only when a material is textured; alpha masks just need the tables
            if ((rc = upload(s, d->textures, d->n_textures, &s->tex.textures))) return bail(rc);
            std::vector<ImageDev> imgs(d->n_images);
            std::vector<float> pool;  // every pyramid, back to back
            for (uint32_t i = 0; i < d->n_images; i++) {
                const rspt_image& im = d->images[i];
                ImageDev& o = imgs[i];
                o.width = im.width; o.height = im.height; o.n_levels = im.n_levels; o.channels = im.channels;
                size_t n_tex = 0;
                for (uint32_t l = 0, w = im.width, h = im.height; l < im.n_levels; l++, w = std::max(1u, w / 2), h = std::max(1u, h / 2)) {
                    o.level_offset[l] = (uint32_t)n_tex;
                    n_tex += (size_t)w * h;
                }
                o.texel_base = pool.size();
                s->image_base.push_back(o.texel_base);
                pool.insert(pool.end(), im.texels, im.texels + n_tex * im.channels);
            }
            if ((rc = upload(s, pool.data(), pool.size(), &s->tex.texel_pool))) return bail(rc);
            if ((rc = upload(s, imgs.data(), imgs.size(), &s->tex.images))) return bail(rc);
            float lut[RSPT_EWA_LUT];  // MipMap::new's EWA weights (mipmap.rs:186-192), host expf like the reference's f32::exp
            for (int i = 0; i < RSPT_EWA_LUT; i++) {
                const float alpha = 2.0f, r2 = (float)i / (float)(RSPT_EWA_LUT - 1);
                lut[i] = std::exp(-alpha * r2) - std::exp(-alpha);
            }
            if ((rc = upload(s, lut, (size_t)RSPT_EWA_LUT, &s->tex.ewa_lut))) return bail(rc);
        }
    }
    if ((rc = upload(s, d->lights, d->n_lights, &s->dev.lights))) return bail(rc);
    {   // Scene.infinite_lights (scene.rs:40-43) and their environment maps
        std::vector<uint32_t> inf;
        for (uint32_t i = 0; i < d->n_lights; i++)
            if (d->lights[i].kind == RSPT_LIGHT_INFINITE) inf.push_back(i);
        s->dev.n_infinite = (uint32_t)inf.size();
        if ((rc = upload(s, inf.data(), inf.size(), &s->dev.infinite_lights))) return bail(rc);
        std::vector<EnvMapDev> envs(d->n_envmaps);
        for (uint32_t i = 0; i < d->n_envmaps; i++) {
            const rspt_envmap& e = d->envmaps[i];
            EnvMapDev& m = envs[i];
            m.width = e.width; m.height = e.height; m.n_levels = e.n_levels; m.nu = e.dist_nu; m.nv = e.dist_nv;
            size_t n_tex = 0;
            for (uint32_t l = 0, w = e.width, h = e.height; l < e.n_levels; l++, w = std::max(1u, w / 2), h = std::max(1u, h / 2)) {
                m.level_offset[l] = (uint32_t)n_tex;
                n_tex += (size_t)w * h;
            }
            if ((rc = upload(s, e.texels, n_tex * 3, &m.texels))) return bail(rc);
            if (!e.dist_func) continue;   // (ABI 24) the map of a projection / goniometric light: the pyramid alone, the distribution pointers stay null
            // Distribution2D::new (sampling.rs:156-170) = Distribution1D::new (:24-49) per row and for the marginal
            const uint32_t nu = e.dist_nu, nv = e.dist_nv;
            std::vector<float> cdf((size_t)nv * (nu + 1)), fint(nv), mcdf(nv + 1);
            auto dist1d = [](const float* f, uint32_t n, float* c) {
                c[0] = 0.0f;
                for (uint32_t k = 1; k <= n; k++) c[k] = c[k - 1] + f[k - 1] / (float)n;
                float fi = c[n];
                if (fi == 0.0f) for (uint32_t k = 1; k <= n; k++) c[k] = (float)k / (float)n;
                else for (uint32_t k = 1; k <= n; k++) c[k] /= fi;
                return fi;
            };
            for (uint32_t v = 0; v < nv; v++) fint[v] = dist1d(e.dist_func + (size_t)v * nu, nu, cdf.data() + (size_t)v * (nu + 1));
            m.marg_int = dist1d(fint.data(), nv, mcdf.data());
            if ((rc = upload(s, e.dist_func, (size_t)nu * nv, &m.cond_func)) || (rc = upload(s, cdf.data(), cdf.size(), &m.cond_cdf)) ||
                (rc = upload(s, fint.data(), fint.size(), &m.cond_int)) || (rc = upload(s, fint.data(), fint.size(), &m.marg_func)) ||
                (rc = upload(s, mcdf.data(), mcdf.size(), &m.marg_cdf)))
                return bail(rc);
        }
        if ((rc = upload(s, envs.data(), envs.size(), &s->dev.envmaps))) return bail(rc);
    }
    s->dev.nodes = reinterpret_cast<const float4*>(nodes_d);
    s->dev.n_nodes = (uint32_t)d->n_nodes; s->dev.n_prims = (uint32_t)d->n_prims; s->dev.n_lights = d->n_lights;
    if (d->n_nodes) {
        for (int i = 0; i < 3; i++) { s->dev.wb_min[i] = d->nodes[0].bmin[i]; s->dev.wb_max[i] = d->nodes[0].bmax[i]; }
    } else {
        for (int i = 0; i < 3; i++) { s->dev.wb_min[i] = RSPT_FLT_MAX; s->dev.wb_max[i] = -RSPT_FLT_MAX; }  // Bounds3f::default
    }
    // ---- four-box records (trace_w4.h): grandchildren of every interior node at even depth; with object instances every object's
    // aggregate gets its own records behind the top-level ones, and every instance primitive the reference to the rest of its leaf ----
    std::vector<uint32_t> obj_root(d->n_objects, RSPT_NONE), inst_cont_h(d->n_instances, RSPT_NONE);
    if (d->n_nodes > 0) {
        std::vector<uint2> big;
        auto range_ref = [&](uint32_t off, uint32_t cnt) -> uint32_t {
            if (cnt <= 15u && off <= RSPT_W4_OFFSET_MASK) return RSPT_REF_LEAF | ((cnt - 1u) << RSPT_W4_COUNT_SHIFT) | off;
            big.push_back(make_uint2(off, cnt));
            return RSPT_REF_LEAF | (15u << RSPT_W4_COUNT_SHIFT) | (uint32_t)(big.size() - 1);
        };
        auto leaf_ref = [&](uint32_t ni) -> uint32_t {
            const rspt_bvh_node& n = d->nodes[ni];
            if (instanced && ni < n_top_nodes)  // an instance in this leaf: the primitives behind it are reached again through its continuation reference
                for (uint32_t i = 0; i + 1u < n.n_prims; i++) {
                    const rspt_prim& p = d->prims[(uint32_t)n.offset + i];
                    if (p.mesh == RSPT_MESH_INSTANCE) inst_cont_h[p.v[0]] = range_ref((uint32_t)n.offset + i + 1u, n.n_prims - i - 1u);
                }
            return range_ref((uint32_t)n.offset, n.n_prims);
        };
        // the records of the tree rooted at LinearBVHNode `root` (an interior node), depth first, with record-local indices
        auto build_tree = [&](uint32_t root, std::vector<Wide4Node>& recs, std::vector<uint32_t>& rec_axes) {
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
                    if (x.n_prims != 0) w.ref[k] = leaf_ref(slot_node[k]);
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
        };
        // final form of a record: child indices through `new_of` (+ base), the three axes in bits 25..26 of the first three refs (an
        // empty slot has a NaN box, its ref is never read as a ref)
        auto finish_rec = [&](Wide4Node w, uint32_t axes, const std::vector<uint32_t>* new_of, uint32_t base) {
            for (int k = 0; k < 4; k++)
                if (w.ref[k] != RSPT_NONE && !(w.ref[k] & RSPT_REF_LEAF)) w.ref[k] = (new_of ? (*new_of)[w.ref[k]] : w.ref[k]) + base;
            for (int k = 0; k < 3; k++) w.ref[k] = (w.ref[k] & ~RSPT_W4_AXIS_MASK) | (((axes >> (2 * k)) & 3u) << RSPT_W4_AXIS_SHIFT);
            return w;
        };
        std::vector<Wide4Node> recs, local;
        std::vector<uint32_t> axes;
        if (d->nodes[0].n_prims != 0) {
            s->w4_root = leaf_ref(0);
        } else {
            build_tree(0u, local, axes);
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
            s->w4_top = (uint32_t)order.size();
            s->w4_root = 0u;
        }
        for (uint32_t o = 0; instanced && o < d->n_objects; o++) {
            const rspt_object& ob = d->objects[o];
            if (ob.n_nodes == 0) obj_root[o] = range_ref((uint32_t)ob.first_prim, 1u);                       // a lone primitive: no box, no aggregate
            else if (d->nodes[ob.first_node].n_prims != 0) obj_root[o] = leaf_ref((uint32_t)ob.first_node);  // a one-leaf aggregate
            else {
                build_tree((uint32_t)ob.first_node, local, axes);
                const uint32_t base = (uint32_t)recs.size();
                for (size_t i = 0; i < local.size(); i++) recs.push_back(finish_rec(local[i], axes[i], nullptr, base));
                obj_root[o] = base;
            }
        }
        // record indices and big-leaf indices must leave bits 25..30 free; larger scenes stay on the two-box kernel
        s->w4_ok = recs.size() <= RSPT_W4_OFFSET_MASK && big.size() <= RSPT_W4_OFFSET_MASK;
        if (s->w4_ok && !recs.empty() && (rc = upload(s, recs.data(), recs.size(), &s->w4))) return bail(rc);
        if (!big.empty() && (rc = upload(s, big.data(), big.size(), &s->big_leaves))) return bail(rc);
        // ---- the quantised form of the records (trace_w4q.h) for the shadow rays of scenes without instances and alpha masks ----
        bool any_alpha = false;
        for (uint32_t i = 0; i < d->n_meshes; i++) any_alpha = any_alpha || d->meshes[i].alpha_tex || d->meshes[i].shadow_alpha_tex;
        // (not for scenes with spheres either: k_trace_w4q walks triangle leaves only, and launch_trace_sph never takes it)
        if (s->w4_ok && !recs.empty() && !instanced && !any_alpha && d->n_spheres == 0 && !quadrics && env_size("RSPT_W4Q_BUILD", 1) != 0) {
            std::vector<Quad4Node> q(recs.size());
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
            if (ok) {
                std::vector<float4> lb(2 * (size_t)d->n_prims, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
                for (uint64_t ni = 0; ni < d->n_nodes; ni++) {
                    const rspt_bvh_node& n = d->nodes[ni];
                    if (n.n_prims == 0) continue;
                    lb[2 * (size_t)n.offset] = make_float4(n.bmin[0], n.bmin[1], n.bmin[2], n.bmax[0]);   // the layout box_hit reads (sc.nodes)
                    lb[2 * (size_t)n.offset + 1] = make_float4(n.bmax[1], n.bmax[2], 0.0f, 0.0f);
                }
                if ((rc = upload(s, q.data(), q.size(), &s->w4q)) || (rc = upload(s, lb.data(), lb.size(), &s->leaf_boxes))) return bail(rc);
            }
        }
    }
    if (d->n_prims) {
        float4* tris = nullptr;
        // a scene with spheres keeps them behind the triangle records (dev_sphere.h SphereDev, RSPT_SPHERE_F4 float4 each)
        const uint64_t n_slots = (uint64_t)d->n_spheres + d->n_disks + d->n_cylinders;   // (disks and cylinders take sphere slots, ABI 27)
        hipError_t e = hipMalloc((void**)&tris, (d->n_prims * 3 + n_slots * RSPT_SPHERE_F4) * sizeof(float4));
        if (e != hipSuccess) return bail(fail(RSPT_E_NOMEM, "triangle records: %s", hipGetErrorString(e)));
        s->allocs.push_back(tris);
        const uint32_t* inst_cont_d = nullptr;
        if ((rc = upload(s, inst_cont_h.data(), inst_cont_h.size(), &inst_cont_d))) return bail(rc);
        // alpha masks in the in-line form (dev_scene.h AlphaMask; kernels.h alpha_simple): possible when every mask of the scene is a ConstantTexture or an
        // ImageTexture under a UVMapping2D with finite parameters, and meshes with uvs have their per-primitive copies (tri_nuv)
        const uint32_t* mesh_mask_d = nullptr;
        if (s->has_alpha && env_size("RSPT_ALPHA_SIMPLE", 1) != 0) {
            std::vector<AlphaEntry> entries;
            std::vector<uint32_t> mesh_mask(d->n_meshes, 0u);
            std::map<std::pair<uint32_t, uint32_t>, uint32_t> seen;
            bool simple = s->image_base.size() == d->n_images;
            auto mask_of = [&](uint32_t tex_plus_1, AlphaMask* m) {
                memset(m, 0, sizeof *m);
                if (!tex_plus_1) return true;
                const rspt_texture& tx = d->textures[tex_plus_1 - 1u];
                if (tx.kind == RSPT_TEX_CONSTANT) { m->kind = 1u; m->value = tx.value[0]; return true; }
                if (tx.kind != RSPT_TEX_IMAGE || tx.mapping != RSPT_MAP_UV || tx.image >= d->n_images) return false;
                for (int k = 0; k < 4; k++) if (!std::isfinite(tx.map[k])) return false;   // (0 * su must be 0: the lookup's zero differentials)
                const rspt_image& im = d->images[tx.image];
                if (!im.n_levels || im.n_levels > 27u) return false;   // (level = n_levels - 1 + log2(1e-8) must be negative: mipmap.rs:236-239)
                m->kind = 2u; m->su = tx.map[0]; m->sv = tx.map[1]; m->du = tx.map[2]; m->dv = tx.map[3];
                m->width = im.width; m->height = im.height; m->wrap = tx.wrap; m->channels = im.channels; m->base = s->image_base[tx.image];
                return true;
            };
            for (uint32_t i = 0; i < d->n_meshes && simple; i++) {
                const rspt_mesh& me = d->meshes[i];
                if (!me.alpha_tex && !me.shadow_alpha_tex) continue;
                if (me.has_uv && d->UV && !s->dev.tri_nuv) { simple = false; break; }
                const auto key = std::make_pair(me.alpha_tex, me.shadow_alpha_tex);
                auto it = seen.find(key);
                if (it == seen.end()) {
                    AlphaEntry e;
                    if (!mask_of(me.alpha_tex, &e.alpha) || !mask_of(me.shadow_alpha_tex, &e.shadow) || entries.size() >= (1u << (32 - MF_MASK_SHIFT))) { simple = false; break; }
                    it = seen.emplace(key, (uint32_t)entries.size()).first;
                    entries.push_back(e);
                }
                mesh_mask[i] = it->second;
            }
            if (simple && !entries.empty()) {
                if ((rc = upload(s, entries.data(), entries.size(), &s->dev.alpha_masks)) || (rc = upload(s, mesh_mask.data(), mesh_mask.size(), &mesh_mask_d))) return bail(rc);
                s->alpha_simple = true;
            }
        }
        hipLaunchKernelGGL(k_build_tris, dim3((uint32_t)((d->n_prims + 255) / 256)), dim3(256), 0, g.stream, s->dev.prims, meshes_d, P_d, (uint32_t)d->n_prims, tris, inst_cont_d, mesh_mask_d);
        e = hipStreamSynchronize(g.stream);
        if (e != hipSuccess) return bail(fail(RSPT_E_HIP, "k_build_tris: %s", hipGetErrorString(e)));
        if (d->n_spheres) {   // ABI 23: the sphere records behind the primitive records (dev_sphere.h SphereDev; k_build_tris wrote the sphere primitives' own records)
            std::vector<SphereDev> sph(d->n_spheres);
            memset(sph.data(), 0, sph.size() * sizeof(SphereDev));
            for (uint32_t k = 0; k < d->n_spheres; k++) sph[k].s = d->spheres[k];
            e = hipMemcpy(tris + 3 * d->n_prims, sph.data(), sph.size() * sizeof(SphereDev), hipMemcpyHostToDevice);
            if (e != hipSuccess) return bail(fail(RSPT_E_HIP, "sphere records: %s", hipGetErrorString(e)));
            s->has_spheres = true;
            s->shade_features |= SF_SPHERE;
            for (uint64_t i = 0; i < d->n_prims; i++)
                if (d->prims[i].mesh == RSPT_MESH_SPHERE && d->prims[i].area_light != -1) s->has_sphere_light = true;
        }
        if (quadrics) {   // ABI 27: every slot again with its kind — the spheres (kind 0, as written above), then the disks, then the cylinders
            std::vector<QuadricDev> q(n_slots);
            memset(q.data(), 0, q.size() * sizeof(QuadricDev));
            for (uint32_t k = 0; k < d->n_spheres; k++) { q[k].s = d->spheres[k]; q[k].kind = QK_SPHERE; }
            for (uint32_t k = 0; k < d->n_disks; k++) { q[d->n_spheres + k].d = d->disks[k]; q[d->n_spheres + k].kind = QK_DISK; }
            for (uint32_t k = 0; k < d->n_cylinders; k++) { q[d->n_spheres + d->n_disks + k].c = d->cylinders[k]; q[d->n_spheres + d->n_disks + k].kind = QK_CYLINDER; }
            e = hipMemcpy(tris + 3 * d->n_prims, q.data(), q.size() * sizeof(QuadricDev), hipMemcpyHostToDevice);
            if (e != hipSuccess) return bail(fail(RSPT_E_HIP, "disk / cylinder records: %s", hipGetErrorString(e)));
            s->has_spheres = s->has_quadrics = true;
            s->has_disks = d->n_disks != 0; s->has_cylinders = d->n_cylinders != 0;
            s->quadric_kinds = s->has_disks && s->has_cylinders ? "disk and cylinder" : (s->has_disks ? "disk" : "cylinder");
            if (disk_light || cylinder_light) {
                s->quadric_light_kinds = disk_light && cylinder_light ? "disk and cylinder" : (disk_light ? "disk" : "cylinder");
                s->quadric_light_what = disk_light && cylinder_light ? "disk area lights and cylinder area lights" : (disk_light ? "disk area lights" : "cylinder area lights");
            }
            s->shade_features |= SF_SPHERE | SF_QUADRIC;
        }
        s->dev.tris = tris;
        if (s->w4_ok && s->w4 && !instanced && (!s->has_alpha || s->alpha_simple) && env_size("RSPT_SERIAL_W4", 1) != 0) {   // the per-lane kernels' traversal (trace_serial.h)
            s->dev.w4 = s->w4; s->dev.w4_big = s->big_leaves; s->dev.w4_root = s->w4_root;
        }
    }
    if (instanced) {  // InstDev records
        std::vector<InstDev> ins(d->n_instances);
        std::vector<InstAnim> anims;
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
            if (in.animated) {   // a moving instance (ABI 20): AnimatedTransform::new's decomposition of the two keys, as for a moving camera
                if (!std::isfinite(in.time[0]) || !std::isfinite(in.time[1]) || !(in.time[1] > in.time[0]))
                    return bail(fail(RSPT_E_INVALID, "instance %u: animated with time[1] <= time[0] or a non-finite key time", i));
                for (int k = 0; k < 16; k++)
                    if (!std::isfinite(in.to_world_end[k]) || !std::isfinite(in.from_world_end[k]))
                        return bail(fail(RSPT_E_INVALID, "instance %u: non-finite end key matrix", i));
                // transform_point divides by the homogeneous weight and the reference asserts it is not zero (transform.rs:505): an end key whose
                // rows 3 are all zero can only produce such weights
                if (in.to_world_end[12] == 0.0f && in.to_world_end[13] == 0.0f && in.to_world_end[14] == 0.0f && in.to_world_end[15] == 0.0f)
                    return bail(fail(RSPT_E_INVALID, "instance %u: end key with a zero homogeneous row", i));
                if (in.from_world_end[12] == 0.0f && in.from_world_end[13] == 0.0f && in.from_world_end[14] == 0.0f && in.from_world_end[15] == 0.0f)
                    return bail(fail(RSPT_E_INVALID, "instance %u: end key inverse with a zero homogeneous row", i));
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
        if (!anims.empty()) {
            if (s->has_alpha && !s->w4_ok) return bail(fail(RSPT_E_UNSUPPORTED, "moving object instances together with alpha-masked meshes in a scene whose records outgrow the four-box kernel"));
            if ((rc = upload(s, anims.data(), anims.size(), &s->dev.inst_anim))) return bail(rc);
            s->has_animated = true;
            s->shade_features |= SF_ANIM;
        }
        if ((rc = upload(s, ins.data(), ins.size(), &s->dev.inst))) return bail(rc);
        s->dev.n_inst = d->n_instances;
        s->dev.inst_fixed = d->instancing_mode == RSPT_INSTANCING_FIXED ? 1u : 0u;
    }
    if (d->n_nodes > 1 && !instanced) {  // pair records: both children's boxes next to each other (trace_wide.h)
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
        if ((rc = upload(s, pairs.data(), pairs.size(), &s->pairs))) return bail(rc);
    }
    *out = s;
    return RSPT_OK;
}

int rspt_scene_destroy(rspt_scene_t s) {
    if (!s) return RSPT_OK;
    if (g.inited) { (void)hipSetDevice(g.device); (void)hipStreamSynchronize(g.stream); }
    for (void* p : s->allocs) (void)hipFree(p);
    delete s;
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
}  // namespace
extern "C" {
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
    if (s->quadric_light_kinds) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive %s: the light distributions are not built for %s yet", s->quadric_light_kinds, s->quadric_light_what);
    if (s->has_sphere_light) return fail(RSPT_E_UNSUPPORTED, "scene with an emissive sphere: the light distributions are not built for sphere area lights yet");
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
