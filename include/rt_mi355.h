/*
 * rt_mi355.h — C ABI of the MI355X-native render path (librt_mi355.so).
 *
 * Drop-in boundary: this library replaces ONE call of the reference,
 *
 *     camera.render(world, lights, &mut buf)          reference src/main.rs:75
 *     pub fn render(self, world: Arc<dyn Hit>,
 *                   lights: Arc<dyn Hit>, buf: &mut Buffer)   src/camera.rs:189
 *
 * i.e. the per-pixel stratified sample loop, closest-hit scene evaluation,
 * material scattering and the light-biased mixture-PDF sampler.  Everything the
 * reference passes as Rust trait objects (`Arc<dyn Hit>`, `Arc<dyn Material>`,
 * `Arc<dyn Sampler>`) is handed over as the flat tables below: the tree of
 * `Hit` nodes is kept as a tree (node table + child-index table), so a host
 * only has to walk its own object graph once and copy numbers.  The library
 * compiles that tree into its own device layout (scene program, SAH BVHs).
 *
 * Plain C: pointers and sizes only, no C++/torch/HIP types in signatures
 * (the optional stream argument is an opaque `void*` = hipStream_t).
 * All matrices are row-major 4x4 (reference src/mat4.rs:10), all reals are
 * f64 like the reference (src/vec4.rs:10).  Errors: every entry point returns
 * RT_OK (0) or a negative RtStatus; rt_last_error() gives the message for the
 * calling thread.  Nothing throws or aborts across this boundary (the
 * reference panics: Cargo.toml:18 `panic = "abort"`, src/camera.rs:244).
 */
#ifndef RT_MI355_H
#define RT_MI355_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_MI355_ABI_VERSION 2  /* 2: RtRenderStats grew (per-kernel times, state bytes, iterations, replica groups) */

typedef enum RtStatus {
    RT_OK = 0,
    RT_E_INVALID = -1,      /* malformed description (bad index, NULL, size)  */
    RT_E_UNSUPPORTED = -2,  /* valid reference scene feature the kernels lack */
    RT_E_DEVICE = -3,       /* HIP runtime failure / no gfx950 device         */
    RT_E_NOMEM = -4
} RtStatus;

/* ---- Hit tree ----------------------------------------------------------- */
/* One entry per reference `dyn Hit` object (src/object.rs:107-115).         */
typedef enum RtNodeType {
    RT_NODE_SPHERE = 1,     /* src/object/sphere.rs     p = center[3], radius            */
    RT_NODE_PLANE = 2,      /* src/object/plane.rs      p = center[3], u[3], v[3] (half-vectors) */
    RT_NODE_MESH = 3,       /* src/object/mesh.rs       mesh = index into meshes         */
    RT_NODE_LIST = 4,       /* src/object/list.rs       children = members, in order     */
    RT_NODE_TRANSFORM = 5,  /* src/object/transform.rs  1 child, transform = index       */
    RT_NODE_BVH = 6,        /* src/object/bvh.rs        2 children (child 1 may be NULL node) */
    RT_NODE_SKY = 7,        /* src/object/sky.rs        material = embedded Emissive     */
    RT_NODE_SUN = 8,        /* src/object/sun.rs        p = direction[3] (normalised by callee) */
    RT_NODE_VOLUME = 9,     /* src/object/volume.rs     1 child = boundary, p[0] = density */
    RT_NODE_NULL = 10       /* src/object/bvh/null_obj.rs                                */
} RtNodeType;

#define RT_PLANE_RENDER_BACKFACE 1u      /* Plane::render_backface, plane.rs:17  */
#define RT_LIST_DISABLE_BOUNDS_CHECK 1u  /* ObjectList::disable_bounds_check, list.rs:23 */

typedef struct RtNode {
    uint32_t type;          /* RtNodeType */
    uint32_t flags;
    int32_t  material;      /* index into materials, -1 if none */
    int32_t  mesh;          /* RT_NODE_MESH: index into meshes */
    int32_t  transform;     /* RT_NODE_TRANSFORM: index into transforms */
    uint32_t first_child;   /* offset into child_indices */
    uint32_t n_children;
    uint32_t _pad;
    double   bounds[6];     /* Hit::get_bounding_box(): min xyz, max xyz (object.rs:110) */
    double   p[12];         /* per-type parameters, see RtNodeType */
} RtNode;

/* Transform::transform / inv_transform after all ops (transform.rs:14-20).  */
typedef struct RtTransform {
    double m[16];
    double inv[16];
} RtTransform;

/* TriangleMesh (mesh.rs:22-35) as loaded by loaders/obj.rs: indexed arrays. */
#define RT_MESH_FLAT_SHADING 1u
#define RT_MESH_HIT_BACK_FACES 2u
typedef struct RtMesh {
    const double*   positions;   /* n_positions * 3 */
    const double*   normals;     /* n_normals * 3 (unit length, obj.rs:48)   */
    const double*   uvs;         /* n_uvs * 3 (u, v, w), may be NULL         */
    const uint32_t* tri_pos;     /* n_triangles * 3 indices into positions   */
    const uint32_t* tri_nrm;     /* n_triangles * 3 indices into normals     */
    const int32_t*  tri_uv;      /* n_triangles * 3 indices into uvs, or -1 (Triangle::uv_indices None); may be NULL */
    uint32_t n_positions, n_normals, n_uvs, n_triangles;
    uint32_t flags;
    uint32_t _pad;
} RtMesh;

/* ---- Materials and textures -------------------------------------------- */
typedef enum RtMaterialType {
    RT_MAT_LAMBERTIAN = 1,   /* material/lambertian.rs  tex_a = albedo                 */
    RT_MAT_METAL = 2,        /* material/metal.rs       tex_a = albedo, tex_b = roughness */
    RT_MAT_DIELECTRIC = 3,   /* material/dielectric.rs  ior                            */
    RT_MAT_GLOSSY = 4,       /* material/glossy.rs      tex_a, tex_b, ior, tex_c = normal map or -1 */
    RT_MAT_EMISSIVE = 5,     /* material/emissive.rs    tex_a = emission map           */
    RT_MAT_ISOTROPIC = 6,    /* material/isotropic.rs   tex_a = albedo                 */
    RT_MAT_NORMAL_DEBUG = 7  /* material/normal_debug.rs tex_c = normal map or -1      */
} RtMaterialType;

typedef struct RtMaterial {
    uint32_t type;
    int32_t  tex_a, tex_b, tex_c;
    double   ior;
} RtMaterial;

typedef enum RtTextureType {
    RT_TEX_CONST_COLOR = 1,    /* texture/constant.rs   v = rgb                        */
    RT_TEX_CONST_FLOAT = 2,    /* texture/constant.rs   v[0] = k                       */
    RT_TEX_CHECKER = 3,        /* texture/checkerboard.rs:34  a = even, b = odd, scale */
    RT_TEX_CHECKER_SOLID = 4,  /* texture/checkerboard.rs:74                           */
    RT_TEX_LERP = 5,           /* texture/interpolate.rs  a, b, c = t                  */
    RT_TEX_IMAGE = 6,          /* texture/image.rs:37-53  texels, width, height (repeat, nearest) */
    RT_TEX_NOISE_SOLID = 7,    /* texture/noise.rs:33-38  v = scale vector, samples, perlin_* tables */
    RT_TEX_CHANNEL = 8,        /* texture/channel.rs  a = colour texture, channel      */
    RT_TEX_UV_DEBUG = 9        /* texture/uv_debug.rs                                  */
} RtTextureType;

typedef struct RtTexture {
    uint32_t type;
    int32_t  a, b, c;
    uint32_t channel;
    uint32_t samples;           /* NOISE_SOLID: turbulence octaves (noise.rs:27, default 7)            */
    double   v[3];              /* CONST_*: the value; NOISE_SOLID: NoiseSolidTexture::scale (noise.rs:16) */
    double   scale;
    /* IMAGE: what Buffer::from_image keeps (buffer.rs:30-48): width*height RGB triples as decoded by
     * `into_rgb32f` (8-bit: x/255, 16-bit: x/65535, in f32), row 0 = top row of the file.            */
    const float* texels;
    uint32_t width, height;
    /* NOISE_SOLID: the generator's tables (noise/perlin.rs:13-18). The reference fills them from its
     * entropy-seeded RNG (perlin.rs:21-36); the caller passes its own.                                */
    const double*   perlin_vec;   /* 256 unit vectors, x y z            */
    const uint32_t* perlin_perm;  /* perm_x[256], perm_y[256], perm_z[256], values 0..255 */
} RtTexture;

typedef struct RtSceneDesc {
    uint32_t abi_version;         /* RT_MI355_ABI_VERSION */
    uint32_t n_nodes;
    const RtNode* nodes;
    uint32_t n_child_indices;
    uint32_t n_transforms;
    const uint32_t* child_indices;
    const RtTransform* transforms;
    uint32_t n_meshes;
    uint32_t n_materials;
    const RtMesh* meshes;
    const RtMaterial* materials;
    uint32_t n_textures;
    uint32_t world_root;          /* node index of `world`  (main.rs:75 arg 1) */
    const RtTexture* textures;
    uint32_t lights_root;         /* node index of `lights` (main.rs:75 arg 2) */
    uint32_t flags;               /* RT_SCENE_* */
} RtSceneDesc;

/* RtSceneDesc.flags */
#define RT_SCENE_BVH_ON_DEVICE 1u /* build the mesh BVHs on the GPU (LBVH: milliseconds instead of ~0.7 s per 870k
                                     triangles, slower traversal); default: binned SAH on the host.  The tree only
                                     culls, so the rendered values do not depend on the builder.               */

/* ---- Camera: the fields of `Camera` after init() (camera.rs:19-44,86-130) */
typedef struct RtCameraDesc {
    uint32_t image_width, image_height;
    double position[3];
    double first_pixel[3];
    double pixel_delta_u[3];
    double pixel_delta_v[3];
    double basis_u[3];
    double basis_v[3];
    uint32_t has_aperture;        /* aperture_radius.is_some() */
    uint32_t _pad;
    double aperture_radius;
} RtCameraDesc;

typedef enum RtPrecision { RT_PRECISION_F64 = 0, RT_PRECISION_F32 = 1 } RtPrecision;
typedef enum RtPipeline { RT_PIPELINE_AUTO = 0, RT_PIPELINE_MEGAKERNEL = 1, RT_PIPELINE_WAVEFRONT = 2 } RtPipeline;

/* Render parameters: CameraConfig (config.rs:46-52) + the additions a
 * deterministic, shardable renderer needs (seed, row partition, precision). */
typedef struct RtRenderParams {
    uint32_t sqrt_spt;            /* Camera::sqrt_spt: strata per axis per replica         */
    uint32_t thread_count;        /* Camera::thread_count: number of sample replicas (NOT OS threads) */
    uint32_t max_depth;           /* config.rs:76 default 20                               */
    uint32_t has_background;      /* Camera::background_color.is_some()                    */
    double   light_bias;          /* config.rs:77 default 0.25                             */
    double   background[3];
    uint64_t seed;                /* new: the reference seeds from OS entropy (camera.rs:208) */
    /* Row partition for multi-GPU rendering: rows are grouped in bands of
     * `band_rows`; band b belongs to part (b % n_parts).  band_rows == 0 or
     * n_parts <= 1 means "whole frame".  Output holds only the owned rows,
     * packed in increasing y.                                               */
    uint32_t band_rows;
    uint32_t n_parts;
    uint32_t part;
    uint32_t precision;           /* RtPrecision: arithmetic type of the kernels */
    uint32_t pipeline;            /* RtPipeline */
    uint32_t collect_stats;       /* count node visits / triangle tests / rays (slower) */
} RtRenderParams;

/* Counters and timings of the last rt_render* call on a scene. */
typedef struct RtRenderStats {
    double   kernel_ms;           /* HIP-event time of all render kernels of the call (their own stream) */
    double   traversal_kernel_ms; /* of which: dominant kernel (megakernel, or wavefront intersect)      */
    uint32_t n_launches;          /* stand-alone launches of the search kernel that opens an iteration (k_wf_prims /
                                     k_wf_intersect; the megakernel: 1): n_iterations unless k_wf_shade runs the search */
    uint32_t pipeline_used;       /* RtPipeline actually run                                             */
    uint64_t samples;             /* W * owned_rows * spp                                                */
    uint64_t rays;                /* world.test() calls (closest-hit casts); valid if collect_stats      */
    uint64_t mesh_rays;           /* casts that entered a mesh BVH                                       */
    uint64_t node_visits;         /* mesh-BVH nodes fetched                                              */
    uint64_t tri_tests;           /* Moller-Trumbore tests                                               */
    uint64_t prim_tests;          /* sphere/quad/sky/sun tests incl. light-pdf re-intersections          */
    uint64_t bytes_node;          /* bytes per BVH node in the layout used                               */
    uint64_t bytes_tri;           /* bytes per triangle record                                           */
    uint64_t bytes_attr;          /* bytes of shading attributes fetched per mesh hit                    */
    uint64_t bytes_state;         /* bytes of path state the traversal kernel moves per ray it handles (0: megakernel) */
    /* wavefront scheduler only (0 otherwise): HIP-event sums per kernel of the iteration loop, and the
     * algorithmic path-state bytes (read + written) per ray that passes through each of them              */
    double   prims_kernel_ms;     /* k_wf_prims (stand-alone launches): scene program over spheres / quads / sky / sun */
    double   shade_kernel_ms;     /* k_wf_shade: scatter, pdf, regeneration, queue compaction (+ the search when fused) */
    uint64_t bytes_state_prims;
    uint64_t bytes_state_shade;
    uint32_t n_iterations;        /* wavefront iterations (one bounce of every live path each)             */
    uint32_t n_replica_groups;    /* groups the replicas were rendered in (per-sample buffer budget)       */
    uint32_t n_tail_compactions;  /* times the live paths were moved together at the end of a group (k_wf_compact) */
    uint32_t _reserved;
} RtRenderStats;

typedef struct RtScene RtScene;

/* Number of usable gfx950 devices (0 if none; never fails). */
int rt_device_count(void);

/* Deep-copies `desc`, builds the device scene (scene program, per-mesh SAH
 * BVH) and uploads it to device `device`.  Replaces the construction of the
 * `Arc<dyn Hit>` graph as far as the render path is concerned.              */
int rt_scene_create(const RtSceneDesc* desc, int device, RtScene** out);
void rt_scene_destroy(RtScene* scene);

/* ---- Updating a scene in place: same structure, new numbers ------------------------------------------
 * rt_scene_update gives `scene` the numbers of `desc`, which must describe the same structure as the description the
 * scene holds: equal counts, roots, child_indices; per node type / flags / material / mesh / transform / first_child /
 * n_children; per mesh the four counts, flags, the contents of tri_pos / tri_nrm / tri_uv and which arrays are present;
 * per material type / tex_a / tex_b / tex_c; per texture type / a / b / c / channel / samples / width / height and which
 * tables are present.  Free to change: RtNode.bounds and .p, every RtTransform, the meshes' positions / normals / uvs,
 * RtMaterial.ior, RtTexture.v / .scale / texels / noise tables.  desc->flags is ignored (nothing is built).
 * Anything else is RT_E_INVALID with a message naming the first field that differs; a description rt_scene_create
 * refuses is refused with the same status (mesh coordinates that are not finite or beyond 1e37: RT_E_UNSUPPORTED); in
 * both cases the scene is unchanged: everything the host can check is checked before device state is touched.
 * After RT_OK every entry point behaves as for a scene freshly created from `desc`, in both precisions and pipelines
 * (frames equal bit for bit, up to ties between two triangles hit at exactly equal t, which two different trees may
 * resolve differently).  The mesh BVHs keep their trees: per mesh whose vertex arrays differ bytewise from the scene's,
 * only those arrays are copied to the device, and kernels rewrite the triangle records, the boxes of every node format
 * and the back-face cones in place; meshes whose arrays are equal cost nothing.  The scene program, primitive groups,
 * lights, materials and textures are recompiled on the host and uploaded again.  A tree refitted far from the shape it
 * was built for culls worse (never wrongly): re-create the scene when that matters.
 * Synchronous, on the scene's own stream; must not overlap a render of the same scene.  Accumulators created before the
 * update belong to the old scene: every call on them but rt_accum_destroy returns RT_E_INVALID.  An RT_E_DEVICE from
 * the refit kernels themselves leaves the mesh tables undefined: destroy the scene.                                    */
typedef struct RtSceneUpdateInfo {
    uint32_t n_meshes_refit;      /* distinct meshes whose positions / normals / uvs differed from the scene's current ones */
    uint32_t n_triangles_refit;
    uint64_t bytes_uploaded;      /* vertex arrays + (first time a mesh moves) its index arrays + small tables + texels */
    double   refit_kernel_ms;     /* HIP-event time of the refit kernels (0 when no mesh changed or nothing is on the device yet) */
    double   total_ms;            /* host clock around the whole call, device synchronise included */
    uint32_t _reserved[4];        /* zero */
} RtSceneUpdateInfo;
int rt_scene_update(RtScene* scene, const RtSceneDesc* desc, RtSceneUpdateInfo* info_or_null);
/* Host only: RT_OK if `b` has the structure of `a`, else RT_E_INVALID with the message rt_scene_update would give. */
int rt_scene_update_check(const RtSceneDesc* a, const RtSceneDesc* b);
/* Host only: the refit restated on the CPU.  The tree rt_scene_create(a) builds for mesh INSTANCE `mesh`, carrying the
 * geometry of `b` (same structure as `a`): outputs as rt_scene_mesh_cones (children relative to the mesh, cone words),
 * plus boxes_out[24 i + 6 k ..] = the decoded quantised box of child k of node i as six floats (org + q cell: lo xyz,
 * hi xyz; an empty child has lo > hi), tris_out = the records in the kernels' arithmetic type widened to double, and
 * tri_order_out[slot] = the original triangle of leaf slot `slot`.  Any output pointer may be NULL.                 */
int rt_scene_refit_mesh(const RtSceneDesc* a, const RtSceneDesc* b, uint32_t mesh, uint32_t f32, int32_t* children_out,
                        uint32_t* cones_out, float* boxes_out, uint32_t node_capacity, uint32_t* n_nodes_out,
                        double* tris_out, uint32_t* tri_order_out, uint32_t tri_capacity, uint32_t* n_tris_out);
/* The same outputs, downloaded from what k_wf_mesh reads on the device for that precision (materialised if needed). */
int rt_debug_scene_mesh(const RtScene* scene, uint32_t mesh, uint32_t f32, int32_t* children_out, uint32_t* cones_out,
                        float* boxes_out, uint32_t node_capacity, uint32_t* n_nodes_out, double* tris_out,
                        uint32_t* tri_order_out, uint32_t tri_capacity, uint32_t* n_tris_out);
/* Diagnostic: digests of the mesh tables as they stand on the device for one precision (materialised if needed):
 * out[0..6] = BvhNode, BvhNode4f, quantised nodes + cones, triangle records, attributes, mesh boxes, mesh op records;
 * out[7] = number of updates so far.  A scene refitted by kernels and one whose tables the host derived from the same
 * tree and vertices give equal digests.                                                                               */
int rt_debug_scene_mesh_digest(const RtScene* scene, uint32_t f32, uint64_t out[8]);
/* The same seven digests of the tables as the host derives them for rt_scene_create(desc) (host only unless the scene
 * asks for the device BVH builder, which runs on the current device); out[7] = 0.  What a fresh scene uploads. */
int rt_scene_tables_digest(const RtSceneDesc* desc, uint32_t f32, uint64_t out[8]);
/* Diagnostic: what the library holds through HIP in this process, over all scenes and accumulators: out[0] = live device
 * buffers, out[1] = their bytes, out[2] = live pinned host buffers, out[3] = live events + streams.  Counted where the
 * library allocates, so other users of the card do not show.                                                          */
int rt_debug_live_resources(uint64_t out[4]);

/* Number of rows the partition in `params` assigns to this part. */
uint32_t rt_owned_rows(uint32_t image_height, const RtRenderParams* params);

/* The replacement for Camera::render (camera.rs:189-256).  Synchronous.
 * rgba_out: caller-allocated, owned_rows * width * 4 doubles, row-major,
 * overwritten with the per-pixel mean linear radiance (r, g, b, 0): exactly
 * what the reference leaves in `buf` (camera.rs:229-231, 247-253).          */
int rt_render(const RtScene* scene, const RtCameraDesc* camera,
              const RtRenderParams* params, double* rgba_out);

/* Same, but the output stays in HBM: d_rgba_out is a device pointer on the
 * scene's device (owned_rows * width * 4 doubles); work is enqueued on
 * `stream` (hipStream_t, NULL = the library's own stream) and the call
 * returns after the kernels complete.                                       */
int rt_render_device(const RtScene* scene, const RtCameraDesc* camera,
                     const RtRenderParams* params, double* d_rgba_out, void* stream);

int rt_get_stats(const RtScene* scene, RtRenderStats* out);

/* Diagnostic probe (tests): traces ONE sample (replica tid, pixel x,y, stratum sx,sy) on the
 * device; rgb_out[3] = its radiance, trace_out[17*max_bounces] = per bounce: t, pos xyz,
 * material index, scene-program op type, triangle slot, 0, normal xyz, ray origin xyz, ray dir xyz.  Returns the bounce count (>= 0)
 * or a negative RtStatus. */
int rt_debug_trace_sample(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params,
                          uint32_t tid, uint32_t x, uint32_t y, uint32_t sx, uint32_t sy,
                          double* rgb_out, double* trace_out, uint32_t max_bounces);

/* Diagnostic probe (tests): the specular reflection of Metal / Glossy (metal.rs:33-35, glossy.rs:66-68) as the kernels compute
 * it - with the shortcut for a fuzz / roughness of exactly 0 - next to the plain expression, on `n` inputs (reflected[3 n],
 * fuzz[n], generator state[n]): out[6 i ..] = the kernels' direction, then the plain one; state_out[2 i ..] = the generator
 * after each.  The two must agree bit for bit. */
int rt_debug_fuzzy_reflection(int device, uint32_t n, const double* reflected, const double* fuzz, const uint64_t* state, double* out, uint64_t* state_out);

/* Diagnostic probe (tests): ONE path vertex for each of n rays, one ray per lane - what one loop trip of the megakernel does
 * to a path with throughput (1,1,1) and radiance 0: the closest-hit search from t_min = 0.001 (with the volumes' free-flight
 * draws), then the shade step, called as the render kernels call them.  rays[6 n]: origin and direction; states[n]: the
 * generator's 64-bit state before the vertex; params: precision and light_bias (and the background) are read.
 * variant 0: the kernel variant the render picks for this scene; 1: the full variant (texture interpreter, volumes, nested
 * light lists); 2: the simple variant, RT_E_INVALID on a scene that needs the full one.
 * out[RT_SHADE_RAYS_STRIDE n], widened to double: [0] t; [1..3] hit position; [4..6] shading normal (after a normal map);
 * [7] u; [8] v ((u, v) stay 0 where no texture of the material reads them); [9] front face; [10] material (-1: a miss);
 * [11] scene-program op type (-1: a miss); [12..14] tex_a; [15] tex_b; [16] 1 if the path continues; [17..19] the
 * continuation direction as computed (not normalised; 0 unless it continues); [20..22] the throughput after the vertex;
 * [23..25] the radiance; [26] the number of draws the search made; [27] 0.  state_out[n]: the generator after the vertex. */
#define RT_SHADE_RAYS_STRIDE 28
int rt_debug_shade_rays(const RtScene* scene, const RtRenderParams* params, uint32_t variant, uint32_t n, const double* rays,
                        const uint64_t* states, double* out, uint64_t* state_out);

/* Diagnostic (host only, needs no device): compiles `desc` like rt_scene_create and reports how the scene
 * compiler classified it.  RT_SCENE_INFO_ZERO_WEIGHT_STOP: the light set cannot give an infinite or NaN weight,
 * so paths whose weight is exactly 0 are ended early (otherwise they are traced to the end like
 * camera.rs:310-314 does); _TEX_INTERPRETER: full-feature kernel variants; _VOLUMES: combined intersect kernel. */
#define RT_SCENE_INFO_ZERO_WEIGHT_STOP 1u
#define RT_SCENE_INFO_TEX_INTERPRETER 2u
#define RT_SCENE_INFO_VOLUMES 4u
int rt_scene_info(const RtSceneDesc* desc, uint32_t* flags_out);
/* Same, plus mesh statistics of the compiled scene (distinct meshes, host-built BVH):
 * out[0] triangle records, out[1] BVH2 nodes, out[2] 4-wide nodes, out[3] BVH2 depth, out[4] worst-case 4-wide traversal stack,
 * out[5] scene-program ops, out[6] sphere / quad groups re-built as SAH trees, out[7] primitives in them. */
int rt_scene_mesh_stats(const RtSceneDesc* desc, uint64_t out[8]);
/* Same, for the back-face cones of k_wf_mesh (tests without a GPU): the 4-wide BVH of mesh instance `mesh` of the compiled scene
 * (instances in program order).  children_out[4 i + k] = child k of node i, node 0 the root: >= 0 inner node, < 0 leaf with
 * ~child = (first triangle << 3) | (count - 1), INT32_MIN no child - all relative to this mesh; cones_out[4 i + k] = that
 * child's cone word, four signed bytes (ax, ay, az, w), built with the conditioning limits of the f64 kernels (f32 = 0) or
 * the f32 kernels (f32 != 0); tris_out[9 t ..] = v0, e1, e2 of triangle t in leaf order (f64 records).  Up to
 * `node_capacity` nodes and `tri_capacity` triangles are written; *n_nodes_out / *n_tris_out = the mesh's totals; the
 * output arrays may be NULL. */
int rt_scene_mesh_cones(const RtSceneDesc* desc, uint32_t mesh, uint32_t f32, int32_t* children_out, uint32_t* cones_out,
                        uint32_t node_capacity, uint32_t* n_nodes_out, double* tris_out, uint32_t tri_capacity, uint32_t* n_tris_out);

/* The normal slabs that k_wf_mesh tests beside the cones, for node i of rt_scene_mesh_cones' order: slabs_out[4 i + k] the
 * word of child k (two signed 16-bit integers: lo | hi << 16; 0x7FFF8000 on a child without a cone), bounds_out[8 i + 2 k + {0, 1}] its decoded [lo, hi],
 * frames_out[4 i + {0, 1, 2}] the node's grid origin and [4 i + 3] its 1 / s: the slab bounds q . (x - org) / s with q the
 * child's three cone axis bytes.  *pad_out: the pad m of the mesh's boxes; the builder widens a slab by |q|_1 (2 m / s + 2^-12).
 * slabs_out NULL: the count only. */
int rt_scene_mesh_slabs(const RtSceneDesc* desc, uint32_t mesh, uint32_t f32, uint32_t* slabs_out, float* bounds_out, float* frames_out,
                        double* pad_out, uint32_t node_capacity, uint32_t* n_nodes_out);
/* The hand-out policy of the persistent search kernels (csrc/rt_handout.h), replayed on the host (tests without a GPU): `waves`
 * waves share a queue of `n` entries and ask for ranges in the order `order` (wave indices; walked round and round, every
 * wave must appear) until each has been told that the queue is exhausted and has asked once more after that.  policy = {mode,
 * left256, left128} or NULL for the default.  asks_out[3 i ..] = wave, first entry, end of the range handed out at ask i
 * (both 0xFFFFFFFF: "exhausted"); up to `capacity` asks are written, *n_asks_out = their number.  atomics_out[0] = atomics on the
 * cursor that the kernel makes, atomics_out[1] = those of the asks after "exhausted" (the kernel makes none). */
int rt_debug_handout_replay(const uint32_t* policy, uint32_t n, uint32_t waves, const uint32_t* order, uint32_t n_order, uint32_t* asks_out,
                            uint32_t capacity, uint32_t* n_asks_out, uint32_t* atomics_out);
/* Same, plus the compiled scene program itself (tests of the scene compiler without a GPU): ops_out[4 * i ..] = type, arg,
 * skip, chain of op i (rt_scene.h OpType; up to `capacity` ops are written, *n_ops_out = the program's length; ops_out may be
 * NULL).  info[0] mesh ops, [1] primitive groups with a 4-wide BVH, [2] their nodes, [3] their worst-case stack, [4] entries of
 * the light table (nested lists flattened to a tree), [5] volumes, [6] the wavefront scheduler's kernel plan: bit 0 split
 * intersect (k_wf_prims + k_wf_mesh), bit 1 volumes inside k_wf_prims, bit 2 multi-mesh form of k_wf_mesh, bit 3 group
 * BVHs in k_wf_prims; [7] primitives in group BVHs. */
int rt_scene_program(const RtSceneDesc* desc, int32_t* ops_out, uint32_t capacity, uint32_t* n_ops_out, uint64_t info[8]);
/* Same, for the 4-wide BVHs of the re-built primitive groups (OP_GROUP) as k_wf_prims reads them, from the derivation that
 * fills the device, in the f64 tables (f32 = 0) or the f32 tables (f32 != 0).  Per group g: roots_out[g] = its root in the
 * scene-wide node array (its nodes run to the next group's root), group_boxes_out[6 g ..] = lo xyz, hi xyz of its box.
 * Per node i: children_out[4 i + k] = child k as the kernel reads it, ABSOLUTE: >= 0 a node of the scene-wide array, < 0 a
 * leaf with ~child = (first position in the scene-wide primitive array << 3) | (count - 1), INT32_MIN no child;
 * boxes_out[24 i + 6 k ..] = that child's decoded quantised box (lo xyz, hi xyz; no child: lo > hi).  Per position j of the
 * primitive array: prims_out[3 j ..] = pc of the primitive's op in the scene program, first entry and length of its run in
 * the guard array; guards_out[] = the guard array (indices of the bounds table).  Every array may be NULL and is written up to
 * its capacity; counts_out[0..5] = groups, nodes, primitive positions, guard entries, stack levels per lane that k_wf_prims
 * is given, entries of the bounds table. */
int rt_scene_groups(const RtSceneDesc* desc, uint32_t f32, uint32_t* roots_out, double* group_boxes_out, uint32_t group_capacity,
                    int32_t* children_out, float* boxes_out, uint32_t node_capacity, int32_t* prims_out, uint32_t prim_capacity,
                    int32_t* guards_out, uint32_t guard_capacity, uint32_t counts_out[6]);

/* Frame pipelining (no counterpart in the reference, which renders one image per process run): while `flag` is set
 * (non-NULL), every rt_render / rt_render_device of this scene object stores 1 to `*flag` as soon as the render can no
 * longer fill the GPU — all samples started, pool slots running empty (wavefront scheduler, last replica group) — and
 * at the latest when the call returns, with or without an error.  A second RtScene created from the same description,
 * driven from another host thread on another stream, can start the NEXT frame at that moment: its full launches run
 * underneath the first render's tail (a chain of small, latency-bound launches: 10 % of a 1/8-frame share).  The caller
 * clears `*flag` before each render.  rust_raytracer_amd.api.FramePipeline and bench.py use it. */
int rt_scene_set_tail_flag(RtScene* scene, int32_t* flag);

/* ---- Progressive, resumable rendering ----------------------------------------------------------------------------
 * A frame with T = thread_count replicas of S^2 = sqrt_spt^2 strata (spp = T S^2) is the ordered sum of per-replica means
 * (camera.rs:229,247-253).  An accumulator holds, after k replicas,
 *
 *     sum_k[p] = sum_{t < k} (sum over the strata of replica t of the radiance) / spp      (f64, added in increasing t)
 *
 * in rt_render's output layout (owned_rows x width x 4 doubles, w = 0; the row partition of `params` is honoured).
 * Every random stream is keyed by (seed, replica, pixel, stratum), so the replicas can be rendered in any number of calls:
 * sum_T is, bit for bit, the frame rt_render returns for the same scene, camera and params, for any split into calls,
 * either pipeline (calls may switch), any replica grouping inside a call, tail compaction on or off, f64 or f32 (within
 * one precision), NaN pixels included.  The estimate at 0 < k <= T is sum_k * (double(T) / double(k)): the frame's
 * expected value from the first k replicas; at k = T the factor is 1.0 and the estimate is the final frame.  At k = 0
 * there is no estimate (RT_E_INVALID).
 *
 * The accumulator keeps its own device buffer: renders of the same RtScene between its calls do not disturb it.  The scene
 * must outlive every call on it but rt_accum_destroy, which may come after rt_scene_destroy.  All calls are synchronous.                                                                        */
typedef struct RtAccum RtAccum;
int rt_accum_create(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, RtAccum** out);
void rt_accum_destroy(RtAccum* acc);
/* Renders the next n_replicas replicas (clamped to T - k; 0 is a no-op).  params_or_null may change pipeline and
 * collect_stats for this call only; any other difference from the creation params is RT_E_INVALID.  rt_get_stats then
 * reports this call (samples = npix * S^2 * n), and the scene's tail flag (rt_scene_set_tail_flag) is set as by
 * rt_render_device, the call's last replica group being its tail.  On an error k is unchanged.  (An adaptive
 * accumulator, see "Adaptive sampling" below, renders only its active pixels and reports the samples it rendered.)    */
int rt_accum_render(RtAccum* acc, uint32_t n_replicas, const RtRenderParams* params_or_null, void* stream);
uint32_t rt_accum_replicas_done(const RtAccum* acc);
int rt_accum_estimate(const RtAccum* acc, double* rgba_out);                           /* host copy of the estimate  */
int rt_accum_estimate_device(const RtAccum* acc, double* d_rgba_out, void* stream);   /* into HBM (scene's device)   */
/* The estimate through rt_tonemap_rgb8_device: owned_rows * width * 3 bytes on the host (a preview copies 3 B per pixel). */
int rt_accum_preview_rgb8(const RtAccum* acc, uint8_t* rgb_out);
/* State blob: a 48-byte little-endian header (magic "RTACCUM\0", u32 format version 1, precision, width, owned rows, T, k,
 * u64 digest of the scene description's content, u64 digest of the camera and of the params fields that change the frame:
 * all but pipeline and collect_stats), then sum_k as owned_rows * width * 4 doubles.  rt_accum_load_state refuses
 * (RT_E_INVALID, a message naming the mismatch, the accumulator unchanged) a truncated blob, a wrong magic or version, and
 * any digest, size, T or precision mismatch.  The scene digest is computed once by rt_scene_create over every array the
 * description points at (texels and Perlin tables included), never over pointer values.                              */
size_t rt_accum_state_size(const RtAccum* acc);
int rt_accum_save_state(const RtAccum* acc, void* buf, size_t size);
int rt_accum_load_state(RtAccum* acc, const void* buf, size_t size);
/* The output stage of rth_tonemap_rgb8 (ACES fit, sRGB OETF, `(x * 255.999) as u8`) on device `device`: d_rgba holds
 * width * height RGBA doubles, d_rgb receives width * height * 3 bytes; both in HBM.  Same operations as the host,
 * uncontracted; only pow may differ in its last bit.  Enqueued on `stream` (NULL = the null stream), returns after it. */
int rt_tonemap_rgb8_device(int device, const double* d_rgba, uint32_t width, uint32_t height, uint8_t* d_rgb, void* stream);

/* ---- First-hit AOVs and the edge-avoiding a-trous denoiser ---------------------------------------------------------
 * AOV image: owned_rows x width x 8 doubles per pixel (the row partition of `params` is honoured):
 *     albedo r g b, normal x y z, depth, coverage
 * each the mean over the first n_replicas replicas' samples (n_replicas * S^2 per pixel).  Every sample is keyed and
 * its camera ray built exactly as the render does it, the closest hit is found with the render's own traversal (volume
 * draws included), and no bounce is traced.  Sums are taken per replica, then in replica order; no atomics.
 *   Surface hit:  normal = the shading normal (world space, facing the ray, normal map applied: what NormalDebug shows),
 *                 depth = |hit position - ray origin|, coverage = 1, albedo by material: Lambertian / Metal / Glossy /
 *                 Isotropic: their colour texture; Dielectric: (1, 1, 1); Emissive: its emission on a front face, 0
 *                 on a back face; NormalDebug: the colour it emits.
 *   Environment:  a miss, a Sky hit or a Sun hit.  Albedo = what the frame shows there: the background colour for a
 *                 miss (0 without one), the emission of the Sky / Sun; normal, depth and coverage = 0.
 * n_replicas must be in 1 .. thread_count (else RT_E_INVALID).  Neither call changes rt_get_stats or the tail flag.   */
int rt_render_aov(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, uint32_t n_replicas,
                  double* aov_out);
int rt_render_aov_device(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params, uint32_t n_replicas,
                         double* d_aov_out, void* stream);  /* HBM output on the scene's device; stream NULL = the scene's */

/* Edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of an RGBA f64 image guided by its AOV image, both w x h.
 * Iteration i = 0 .. iterations-1 filters with the 5 x 5 B3-spline taps (1,4,6,4,1)/16 spaced 2^i pixels apart; taps
 * outside the image are skipped.  Tap weight (f32): h * w_c * w_n * w_a * w_z with
 *     w_c = exp(-|c_q - c_p|^2 / (sigma_color^2 * 2^-i))      (1 when the centre colour is not finite)
 *     w_n = exp(-|n_q - n_p|^2 / sigma_normal^2)      w_a = exp(-|a_q - a_p|^2 / sigma_albedo^2)
 *     w_z = exp(-|z_q - z_p| / (sigma_depth * max(z_p, z_q) + 1e-30))
 * The weighted colour and weight sums are f64.  A tap whose colour is not finite, or whose weight is not positive,
 * contributes nothing; a pixel without a contributing tap keeps its value.  With RT_DENOISE_DEMODULATE the colour is
 * divided by the albedo (per channel, where albedo > 1e-3) before the first iteration and multiplied by it after the
 * last.  The guides are packed once per call into f32.  w (alpha) passes through.  iterations = 0: an exact copy.    */
#define RT_DENOISE_DEMODULATE 1u
#define RT_DENOISE_MAX_ITERATIONS 16u
typedef struct RtDenoiseParams {
    uint32_t iterations;          /* 0 .. RT_DENOISE_MAX_ITERATIONS                                                  */
    uint32_t aov_replicas;        /* rt_accum_*_denoised: replicas of the AOV pass the accumulator caches (1 .. T)  */
    uint32_t flags;               /* RT_DENOISE_*                                                                    */
    uint32_t _reserved0;
    double   sigma_color, sigma_normal, sigma_albedo, sigma_depth;  /* > 0 */
    double   _reserved[4];        /* zero */
} RtDenoiseParams;
/* Fills in the defaults. */
int rt_denoise_default_params(RtDenoiseParams* out);
/* Host buffers: rgba w*h*4 doubles, aov w*h*8 doubles (rt_render_aov), out w*h*4 doubles (may be rgba).  dp NULL = the
 * defaults.  Runs on device `device`.                                                                                  */
int rt_denoise(int device, const double* rgba, const double* aov, uint32_t w, uint32_t h, const RtDenoiseParams* dp,
               double* rgba_out);
/* The same on HBM buffers of device `device`, enqueued on `stream` (NULL = the null stream); returns after it.        */
int rt_denoise_device(int device, const double* d_rgba, const double* d_aov, uint32_t w, uint32_t h,
                      const RtDenoiseParams* dp, double* d_rgba_out, void* stream);
/* The accumulator's estimate, denoised (host copy), and the same tone-mapped on the device by rt_tonemap_rgb8_device
 * (3 B per pixel).  On first use the accumulator renders its AOVs with dp->aov_replicas replicas and keeps them until
 * rt_accum_destroy (a call with another aov_replicas renders them again).  The AOVs are not part of the state blob.
 * An accumulator with a row partition is RT_E_INVALID: the filter needs contiguous rows.                             */
int rt_accum_estimate_denoised(const RtAccum* acc, const RtDenoiseParams* dp, double* rgba_out);
int rt_accum_preview_denoised_rgb8(const RtAccum* acc, const RtDenoiseParams* dp, uint8_t* rgb_out);

/* ---- Adaptive sampling: stop converged pixels of a progressive render -----------------------
 * An accumulator that opts in keeps, beside sum[p], the moments s1[p], s2[p] (f64) of the luminance of its per-replica
 * contributions and n[p] (u32), the replicas in sum[p].  When replica t is added to pixel p, with c the three values the
 * resolve step adds to sum[p] (unchanged):  y = double(T) * ((0.2126 c_r + 0.7152 c_g) + 0.0722 c_b),  s1 += y,  s2 += y y,
 * n += 1, in replica order, f64, uncontracted.
 * Decision points D = { k : min_replicas <= k < T, (k - min_replicas) mod check_interval = 0 }.  When the replica count k
 * reaches one, for every active pixel (all have n = k):
 *     mean = s1 / k;  num = max(s2 - s1 mean, 0);  se2 = num / (double(k) double(k - 1));  lim = threshold (mean + floor);
 *     quiet = se2 <= lim lim          (false when anything is NaN: a pixel whose sums hold a NaN never stops)
 * and a pixel STOPS iff it is quiet and every ACTIVE pixel with |dx|, |dy| <= radius inside the image is quiet too.  A
 * stopped pixel never restarts and does not hold its neighbours.  Decisions depend on the sums alone, so the state does not
 * depend on how the replicas are split into calls (rt_accum_render splits its range at decision points itself), on replica
 * groups, pool size, tail compaction or a save / load in between.  For every pixel sum[p] is, bit for bit, the sum of a
 * plain accumulator after n[p] replicas, n[p] in D or = T; without a decision point (min_replicas >= T) the final frame is
 * rt_render's.  Estimate: sum[p] * (double(T) / double(n[p])).  The frame is finished when k = T or no pixel is active;
 * rt_accum_render then renders nothing and returns RT_OK.  rt_get_stats().samples counts what the call really rendered.
 * Adaptive passes run the wavefront scheduler: RT_PIPELINE_MEGAKERNEL or collect_stats in a render call, and max_depth = 0,
 * are RT_E_UNSUPPORTED; a row partition is RT_E_INVALID (the window needs contiguous rows).  On an error inside a call the
 * accumulator keeps the segments (up to a decision point each) that were completed.                                    */
typedef struct RtAdaptiveParams {
    double   threshold;           /* > 0: relative standard error of the luminance at which a pixel is quiet; no default */
    double   floor;               /* > 0: added to the mean, so that dark pixels can converge                          */
    uint32_t min_replicas;        /* >= 2: first decision point                                                         */
    uint32_t check_interval;      /* >= 1: replicas between decision points                                             */
    uint32_t radius;              /* 0 .. 4: half width of the window                                                   */
    uint32_t _reserved0;
    double   _reserved[4];        /* zero */
} RtAdaptiveParams;
/* floor 0.01, min_replicas 4, check_interval 2, radius 1; threshold 0: it must be set by the caller. */
int rt_adaptive_default_params(RtAdaptiveParams* out);
/* Opts in.  Only while no replica has been rendered and no state loaded (else RT_E_INVALID). */
int rt_accum_set_adaptive(RtAccum* acc, const RtAdaptiveParams* params);
uint32_t rt_accum_active_pixels(const RtAccum* acc);   /* plain accumulator: all pixels while k < T, then 0 */
int rt_accum_finished(const RtAccum* acc);             /* 1: k = T or no active pixel */
/* n[p], owned_rows * width values on the host (a plain accumulator: k everywhere). */
int rt_accum_sample_counts(const RtAccum* acc, uint32_t* counts_out);
/* Noise image sqrt(se2) / (mean + floor) per pixel at its n (0 while n < 2); adaptive accumulators only. */
int rt_accum_noise(const RtAccum* acc, double* noise_out);
/* State blob of an adaptive accumulator: format version 2 = the 48-byte header with version 2, 32 bytes of parameters
 * (threshold, floor as f64; min_replicas, check_interval, radius, 0 as u32), then sum (4 f64), s1, s2 (f64) and n (u32)
 * per pixel, array after array.  A plain accumulator still writes version 1.  rt_accum_load_state refuses a version-1
 * blob for an adaptive accumulator, a version-2 blob for a plain one, and parameters that differ.                     */

/* ---- Light groups: one frame per emitter (set) from one render, re-mixed on the device ------
 * A sample's value is one product W * T (weight of the path times the value of its terminal), and only an Emissive
 * material, a NormalDebug material or the background colour give a non-zero T: every sample belongs to exactly one
 * emitter.  A light-group description gives a group id in 0 .. n_groups-1 to every material (material_group[n_materials]),
 * to the background (background_group) and to the black terminals (unlit_group).  The group of a sample is
 *     material_group[m]   its path ends on material m of type Emissive (front or back face; Sky and Sun end on their
 *                         embedded material) or NormalDebug;
 *     background_group    its path misses the scene and the params have a background colour;
 *     unlit_group         every other ending: Absorbed, depth exhausted, a miss WITHOUT a background colour, and a path
 *                         the kernels end early because its weight is zero or NaN in every channel.
 * Entries of material_group that belong to scattering materials are never read.  A non-finite sample goes to its
 * terminal's group like any other.
 * Group frame g = the ordered sum of the frame (per replica the strata in order, / spp, then the replicas in order:
 * camera.rs:229,247-253) with every sample of another group replaced by +0.0: same additions, same order, no atomics.
 * groups_out: n_groups x owned_rows x width x 4 doubles, group-major, w = 0; the row partition of `params` is honoured.
 *   1. The ordinary frame of the same call (rgba_out, may be NULL) is rt_render's, bit for bit, f64 and f32.
 *   2. Group frame g equals, bit for bit where that frame is finite, rt_render's frame of the scene in which every
 *      emitter outside g emits zero - in f64 and f32, for any replica grouping, pool size, tail compaction on or off.
 *   3. Where every sample is >= 0 and the pixel finite, sum_g frame_g (added in group order) differs from the frame by
 *      at most (S^2 + T + G + 2) 2^-52 relative per channel; the union of the groups' non-finite masks is the frame's.
 * Wavefront scheduler only: RT_PIPELINE_MEGAKERNEL, collect_stats and max_depth = 0 are RT_E_UNSUPPORTED.  n_groups outside
 * 1 .. RT_LIGHT_GROUPS_MAX, a NULL table, n_materials other than the scene's and a group id >= n_groups are RT_E_INVALID
 * with a message naming the field; the outputs are then untouched.  rt_get_stats and the tail flag: as rt_render_device.
 * The per-sample buffer takes 25 B per sample (24 B of radiance + the group byte).                                      */
#define RT_LIGHT_GROUPS_MAX 16u
typedef struct RtLightGroups {
    uint32_t n_groups;              /* 1 .. RT_LIGHT_GROUPS_MAX                    */
    uint32_t n_materials;           /* must equal the scene's                      */
    const uint8_t* material_group;  /* n_materials ids                             */
    uint32_t background_group, unlit_group;
    uint32_t _reserved[4];          /* zero */
} RtLightGroups;
/* Automatic assignment (host only, needs no device; deterministic).  Group 0 is the unlit group and takes every
 * material that does not emit and NormalDebug.  Each Emissive material that a node reachable from `world_root`
 * references (Sky / Sun: their embedded material) gets the next id, in ascending material index; with has_background the
 * background gets the id after the last of them (else *background_group_out = 0).  Ids that would reach max_groups or
 * more all become max_groups - 1.  material_group_out: n_materials bytes.  *n_groups_out = highest id used + 1.
 * max_groups outside 1 .. RT_LIGHT_GROUPS_MAX: RT_E_INVALID.                                                          */
int rt_light_groups_auto(const RtSceneDesc* desc, uint32_t max_groups, int has_background, uint8_t* material_group_out,
                         uint32_t* background_group_out, uint32_t* n_groups_out);
int rt_render_light_groups(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params,
                           const RtLightGroups* groups, double* groups_out, double* rgba_out_or_null);
/* Outputs in HBM on the scene's device; stream NULL = the scene's own.  Returns after the kernels complete. */
int rt_render_light_groups_device(const RtScene* scene, const RtCameraDesc* camera, const RtRenderParams* params,
                                  const RtLightGroups* groups, double* d_groups_out, double* d_rgba_out_or_null, void* stream);
/* Re-mix: out = (((tint_0 * f_0) + tint_1 * f_1) + ...) per channel (f64, uncontracted, in group order), w = 0.
 * groups: n_groups x h x w x 4 doubles (group-major), tints: n_groups x 3 doubles ON THE HOST in both forms, out: h x w x 4.
 * A tint of exactly 0 switches its group off: its term is +0.0, the product is not formed (0 * inf and 0 * NaN would
 * be NaN).  The result goes through rt_tonemap_rgb8_device for previews.                                              */
int rt_light_mix(int device, const double* groups, uint32_t n_groups, uint32_t w, uint32_t h, const double* tints,
                 double* rgba_out);
int rt_light_mix_device(int device, const double* d_groups, uint32_t n_groups, uint32_t w, uint32_t h, const double* tints,
                        double* d_rgba_out, void* stream);

/* ---- Ray queries: closest hit and occlusion for rays of the caller's own ----------------------
 * Picking, visibility and occlusion baking, line-of-sight tests, collision probes: n rays against the scene as it stands
 * (after rt_scene_update: the new numbers).  General rules: n = 0 is a no-op; a NULL array is RT_E_INVALID; a precision
 * other than RT_PRECISION_F64 / _F32 is RT_E_INVALID; a scene whose program contains volumes (RT_SCENE_INFO_VOLUMES) is
 * RT_E_UNSUPPORTED (a medium gives no deterministic surface: Volume::test draws from a path's generator).  Non-finite ray
 * components are not an error: the result for such a ray is whatever the arithmetic gives.  Synchronous, like the renders;
 * must not overlap a render or an update of the same scene.  rt_get_stats and the tail flag are left alone.  The workspace
 * (a path pool of RT_RQ_CHUNK rays, environment variable, default 2^22; larger batches run in chunks) belongs to the scene,
 * is allocated by the first query, is separate from the render's pool and is freed by rt_scene_destroy.                  */
#define RT_RAY_HIT          1u   /* something was hit (surface or environment) */
#define RT_RAY_FRONT_FACE   2u   /* HitRecord::front_face */
#define RT_RAY_ENVIRONMENT  4u   /* the hit is a Sky (t = +inf) or a Sun (t = DBL_MAX), as the reference reports them */
typedef struct RtRayHit {        /* 96 bytes */
    double   t;                  /* miss: +inf, flags = 0, ids = -1, the other reals 0 */
    double   pos[3], normal[3];  /* HitRecord::hit_pos / ::normal as the reference leaves them after Transform::test:
                                    world space, facing against the ray, BEFORE any normal map */
    double   u, v;               /* HitRecord::u, ::v, always computed (not only when the material reads them) */
    int32_t  material;           /* index into RtSceneDesc.materials */
    int32_t  node;               /* index into RtSceneDesc.nodes of the Sphere / Plane / Mesh / Sky / Sun node that was hit */
    int32_t  prim;               /* Mesh: triangle index in RtMesh.tri_pos order (NOT the leaf slot); else -1 */
    uint32_t flags;              /* RT_RAY_* */
    uint64_t _reserved;          /* zero */
} RtRayHit;
typedef struct RtRayQueryStats {
    double   kernel_ms;          /* HIP-event time of the query's kernels, all chunks (copies of the host variants excluded) */
    uint64_t rays;
    uint32_t n_chunks, precision;
    uint32_t _reserved[4];
} RtRayQueryStats;

/* Closest hit of world.test(ray, Interval(0.001, inf)) - the interval every ray of the render is cast with - for n caller
 * rays: origins / dirs = n x 3 doubles; directions need not be unit length, t is in units of |dir|.  The scene's own search
 * kernels run, chosen as a render chooses them, so ties are the render's (equal t: the primitive the reference visits
 * first; two triangles at exactly equal t: either).                                                                   */
int rt_trace_rays(const RtScene* scene, uint64_t n, const double* origins, const double* dirs, uint32_t precision, RtRayHit* hits_out);
/* Device pointers on the scene's device; stream NULL = the scene's own.  Returns after the kernels complete. */
int rt_trace_rays_device(const RtScene* scene, uint64_t n, const double* d_origins, const double* d_dirs, uint32_t precision,
                         RtRayHit* d_hits_out, void* stream);
/* out[i] = 1 iff a Sphere, Plane or mesh triangle is hit inside Interval(t_min[i], t_max[i]) (both ends excluded); Sky and
 * Sun never occlude.  t_min NULL = 0.001 for every ray, t_max NULL = +inf.  The hit is not identified and need not be the
 * nearest: the answer is 1 iff some primitive's own reference test accepts inside the interval and every reference
 * ancestor box of that primitive passes the reference's box test with that same interval.                             */
int rt_occluded(const RtScene* scene, uint64_t n, const double* origins, const double* dirs, const double* t_min, const double* t_max,
                uint32_t precision, uint8_t* out);
int rt_occluded_device(const RtScene* scene, uint64_t n, const double* d_origins, const double* d_dirs, const double* d_t_min,
                       const double* d_t_max, uint32_t precision, uint8_t* d_out, void* stream);
int rt_ray_query_stats(const RtScene* scene, RtRayQueryStats* out);   /* of the last query on this scene */
/* Host only, needs no device: nodes_out[pc] = RtSceneDesc.nodes index that op pc of the compiled program came from (-1 for
 * ops that belong to no single node), laid out like rt_scene_program's ops: up to `capacity` entries are written,
 * *n_ops_out = the program's length; nodes_out may be NULL.                                                            */
int rt_scene_op_nodes(const RtSceneDesc* desc, int32_t* nodes_out, uint32_t capacity, uint32_t* n_ops_out);

/* ---- Point queries: the closest surface point and its distance ---------------------------------
 * Probe clearance, snapping points onto a surface, proximity tests, distance fields: for n points q the nearest candidate
 * primitive of the scene as it stands.  Candidates: every Sphere, every Plane (the parallelogram center +- u +- v) and
 * every mesh triangle reachable from the world root, each under its transform chain; Sky and Sun never; the facing flags
 * (RT_MESH_HIT_BACK_FACES, RT_PLANE_RENDER_BACKFACE) do not matter.  The answer is the candidate with the smallest
 * Euclidean world distance, if that distance is strictly below max_distance[i]; at equal distance any of the tied
 * primitives (a mesh vertex is shared by several triangles).  General rules as for the ray queries: n = 0 is a no-op,
 * NULL points / out or a bad precision is RT_E_INVALID, non-finite inputs are not an error, synchronous, must not
 * overlap a render or an update of the scene, rt_get_stats and the tail flag are left alone, chunks of RT_RQ_CHUNK.
 * RT_E_UNSUPPORTED, decided on the host before anything is allocated: a scene with volumes; a scene in which the composed
 * linear part L of the transform chain over a candidate is not a similarity (max|L^T L - s^2 I| <= 1e-9 s^2 with
 * s^2 = tr(L^T L) / 3 is one: only then are object-space distances world distances / s); a mesh BVH deeper than the
 * kernel's LDS stack (64 levels).                                                                                     */
#define RT_POINT_FOUND      1u   /* a primitive lies closer than max_distance */
#define RT_POINT_BACK_SIDE  2u   /* (q - pos) . normal < 0 for the reported primitive */
typedef struct RtPointHit {      /* 80 bytes */
    double   distance;           /* world units; nothing found: +inf, flags 0, ids -1, other reals 0 */
    double   pos[3];             /* the closest point, world space */
    double   normal[3];          /* GEOMETRIC unit normal of the primitive at pos, world space, not flipped towards q: Sphere
                                    away from the centre, (pos - c) / |r|, also for the negative radius of a hollow sphere (the
                                    object-space +x direction when q is the centre), Plane its own normal,
                                    triangle normalize(e1 x e2) (a zero-area triangle: 0) */
    int32_t  material, node, prim;   /* as in RtRayHit: RtSceneDesc indices; prim = triangle in RtMesh.tri_pos order, else -1 */
    uint32_t flags;              /* RT_POINT_* */
    uint64_t _reserved;          /* zero */
} RtPointHit;
/* points: n x 3 doubles; max_distance: n doubles, or NULL = +inf for every point. */
int rt_closest_points(const RtScene* scene, uint64_t n, const double* points, const double* max_distance, uint32_t precision,
                      RtPointHit* out);
/* Device pointers on the scene's device; stream NULL = the scene's own.  Returns after the kernels complete. */
int rt_closest_points_device(const RtScene* scene, uint64_t n, const double* d_points, const double* d_max_distance, uint32_t precision,
                             RtPointHit* d_out, void* stream);
int rt_point_query_stats(const RtScene* scene, RtRayQueryStats* out);   /* of the last point query on this scene; rays = points */
/* Diagnostic, host arrays: counts_out[2i] = BVH nodes visited, counts_out[2i + 1] = triangles tested for point i (the counting
 * variant of the kernel; rt_point_query_stats is left alone). */
int rt_debug_closest_points_counts(const RtScene* scene, uint64_t n, const double* points, const double* max_distance, uint32_t precision,
                                   uint32_t* counts_out);

/* ---- Ambient occlusion at surface points --------------------------------------------------------
 * For point i with position p_i and normal n_i, and sample s = 0 .. samples-1:
 *     generator keyed (seed, 0, i, s) as a render keys (seed, replica, pixel, stratum);
 *     w = n_i / |n_i|, (u, v) the reference's basis about w (utils.rs:17-28), d = u x + v y + w z for the reference's
 *     cosine-weighted (x, y, z) (vec4.rs:50-61, two uniforms);
 *     visible(i, s) = no Sphere, Plane or mesh triangle is hit by p_i + t d inside Interval(bias, max_distance), both ends
 *     excluded: the answer rt_occluded gives for that segment, negated.
 * out[i].visibility = (number of visible samples) / samples, exact; out[i].bent = (sum of d over the visible samples) /
 * samples: the unnormalised bent normal, of length <= 1, 0 for a fully occluded point.  The sum is formed in a fixed order
 * (DESIGN.md section 15), so a call's answer depends on nothing but its arguments and the scene; point i's answer does not
 * depend on n or on the chunk size.  One kernel draws the directions in registers, walks the scene and reduces: no ray is
 * written to memory.  A zero or non-finite normal is not an error: the result is whatever the arithmetic gives.
 * Rules as for the ray queries: n = 0 is a no-op; a NULL array, samples outside 1 .. 4096, a bad precision, a negative or
 * NaN bias, or max_distance <= bias (or NaN) is RT_E_INVALID; a scene with volumes is RT_E_UNSUPPORTED.  Synchronous; must
 * not overlap a render or an update of the same scene; sees the scene as rt_scene_update left it.  rt_get_stats,
 * rt_ray_query_stats and the tail flag are left alone.  Points run in chunks of RT_BAKE_CHUNK (environment variable,
 * default 2^20 points); the host variant's staging buffer belongs to the scene, grows only and is freed by
 * rt_scene_destroy.                                                                                                    */
typedef struct RtBakeParams {    /* NULL = defaults */
    uint32_t samples;            /* per point, 1 .. 4096; default 64 */
    uint32_t precision;          /* RT_PRECISION_F64 / _F32 */
    uint64_t seed;
    double   bias;               /* t_min of every ray, default 0.001 */
    double   max_distance;       /* t_max (directions are unit length); +inf = unlimited (default) */
    uint32_t _reserved[4];
} RtBakeParams;
typedef struct RtBakeResult {    /* 32 bytes */
    double   visibility;
    double   bent[3];
} RtBakeResult;
/* positions / normals: n x 3 doubles each; out: n results. */
int rt_bake_visibility(const RtScene* scene, uint64_t n, const double* positions, const double* normals, const RtBakeParams* params,
                       RtBakeResult* out);
/* Device pointers on the scene's device; stream NULL = the scene's own.  Returns after the kernel completes. */
int rt_bake_visibility_device(const RtScene* scene, uint64_t n, const double* d_positions, const double* d_normals,
                              const RtBakeParams* params, RtBakeResult* d_out, void* stream);
/* The points are hit records on the device (rt_trace_rays_device): pos and normal of record i.  A record without RT_RAY_HIT
 * or with RT_RAY_ENVIRONMENT has no surface point: visibility = 1, bent = 0.                                           */
int rt_bake_visibility_hits_device(const RtScene* scene, uint64_t n, const RtRayHit* d_hits, const RtBakeParams* params,
                                   RtBakeResult* d_out, void* stream);
/* Of the last bake on this scene: rays = n * samples (skipped records included), kernel_ms of the bake kernel alone. */
int rt_bake_stats(const RtScene* scene, RtRayQueryStats* out);

/* ---- Rendering along caller-supplied rays -----------------------------------------------------
 * Radiance per ray: light probes and environment captures, panoramic / orthographic / fisheye views, radiance towards surface
 * points (lightmap and irradiance bakes), reflection captures.  The full path tracer - materials, the light-biased mixture
 * sampler, volumes, every texture - started from n rays of the caller's instead of Camera::get_ray's.
 * origins / dirs: n x 3 doubles each; directions need not be unit length.  rgba_out: n x 4 doubles, (r, g, b, 0) per ray.
 * Of `params`: sqrt_spt (S), thread_count (T), max_depth, has_background / background, light_bias, seed and precision are used.
 * Ray i behaves as pixel i of a frame whose camera sends every sample of that pixel along ray i: sample (t, i, st), t < T,
 * st < S^2, uses the generator keyed (seed, t, i, st) as a render keys (seed, replica, pixel, stratum); its first two uniform
 * draws - a camera's jitter - are drawn and discarded; the path then starts at (origins[i], dirs[i]) with max_depth.  In f32
 * the ray is the table entry rounded to f32.  out[i] is the ordered sum a frame's pixel is: per replica the strata in order,
 * / spp, then the replicas in order; f64, no atomics.  Hence, in f64: out[i] is pixel i of the reference's render with a
 * camera of pixel deltas 0, position = o, first_pixel = o + d (where o + d and (o + d) - o are exact); with S = T = 1 and a
 * camera without aperture the table of that camera's own rays gives rt_render's frame bit for bit; out[i] does not depend on
 * n, the chunk size, the pool size, replica grouping or tail compaction.
 * n = 0 is a no-op.  RT_E_INVALID with a message naming the field: a NULL array, n >= 2^31, n_parts > 1, a bad precision,
 * sqrt_spt or thread_count of 0.  RT_E_UNSUPPORTED, as for light groups: RT_PIPELINE_MEGAKERNEL, collect_stats, max_depth = 0
 * (RT_PIPELINE_AUTO runs the wavefront scheduler).  A scene with volumes is supported.  Non-finite ray components are not an
 * error.  On any error the output is untouched.  rt_get_stats and the tail flag: as rt_render_device, samples = n T S^2.
 * Synchronous; must not overlap a render or an update of the same scene (the render's workspace is used); sees the scene as
 * rt_scene_update left it.  Rays run in chunks of RT_RAYS_CHUNK (environment variable, default 2^22 rays, at most 2^28), each
 * rendered like a frame of that many pixels: inside a chunk the replicas are grouped by the per-sample buffer budget; the
 * generators are keyed by the global index i.  The host variant's staging buffer belongs to the scene, grows only and is
 * freed by rt_scene_destroy.                                                                                            */
int rt_render_rays(const RtScene* scene, uint64_t n, const double* origins, const double* dirs, const RtRenderParams* params,
                   double* rgba_out);
/* Device pointers on the scene's device; stream NULL = the scene's own.  Returns after the kernels complete. */
int rt_render_rays_device(const RtScene* scene, uint64_t n, const double* d_origins, const double* d_dirs,
                          const RtRenderParams* params, double* d_rgba_out, void* stream);

/* ---- Irradiance at surface points ---------------------------------------------------------------
 * Lightmap and vertex-colour bakes, irradiance caches, "clay" previews: the full path tracer - materials, the light-biased
 * mixture sampler, volumes, every texture - started from n surface points in cosine-weighted directions about their normals.
 * One fused pass: the directions are formed in registers, 48 B in and 32 B out per POINT, no ray table.
 * positions / normals: n x 3 doubles each; normals need not be unit length.  rgba_out: n x 4 doubles, (r, g, b, 0) per point.
 * Of `params`: sqrt_spt (S), thread_count (T), max_depth, has_background / background, light_bias, seed and precision are used;
 * R = double or float by the precision.  For point i (its index in the whole call), replica t < T, stratum st = sy S + sx:
 *     Rng g keyed (seed, t, i, st) as a render keys (seed, replica, pixel, stratum);
 *     r1, r2 = the generator's first two uniforms - the two draws a camera spends on its jitter;
 *     u1 = (R(sx) + r1) * inv_S,  u2 = (R(sy) + r2) * inv_S              (inv_S = R(1.0 / double(S)), as the camera forms it)
 *     c = (cos(phi) sqrt(u2), sin(phi) sqrt(u2), sqrt(1 - u2)),  phi = u1 * 2 * pi       (vec4.rs:50-61 with u1, u2 for its draws)
 *     w = R(normal_i) / |R(normal_i)|,  (u, v) the reference's basis about w (utils.rs:17-28),  d = u c.x + v c.y + w c.z + 0 * 0
 *     o = R(pos_i),  d' = (o + d) - o     (two roundings per component: what the reference's camera returns for position = o,
 *                                          first_pixel = o + d, pixel deltas 0, no aperture)
 *     the path starts at (o, d') with max_depth, on g as it now stands: its first draw is the third of the stream, as in a frame.
 * The first segment has the path's usual t_min = 0.001, like a scattered ray leaving a hit; there is no bias parameter.
 * out[i] is the ordered sum a frame's pixel is: per replica the strata in order, / (S^2 T), then the replicas in order; f64, no
 * atomics.  It is the cosine-weighted mean of the incoming radiance: irradiance = pi * out, the outgoing radiance of a
 * Lambertian texel = albedo * out; no factor is applied on the device.  Hence, in f64, sample (t, i, st) is the reference's
 * sample (t, pixel i, st) with that camera, and out[i] does not depend on n, the chunk size, the pool size, replica grouping or
 * tail compaction.  A zero or non-finite normal is not an error: the result is what the arithmetic gives.
 * Rules, stats and the tail flag: rt_render_rays's.  n = 0 is a no-op.  RT_E_INVALID with a message naming the field: a NULL
 * array, n >= 2^31, n_parts > 1, a bad precision, sqrt_spt or thread_count of 0.  RT_E_UNSUPPORTED: RT_PIPELINE_MEGAKERNEL,
 * collect_stats, max_depth = 0.  Everything is checked before the device is touched; on any error the output is untouched.
 * A scene with volumes is supported.  rt_get_stats: samples = n T S^2.  Synchronous; must not overlap a render or an update of
 * the same scene; sees the scene as rt_scene_update left it.  Points run in chunks of RT_RAYS_CHUNK, like rays.             */
int rt_bake_irradiance(const RtScene* scene, uint64_t n, const double* positions, const double* normals, const RtRenderParams* params,
                       double* rgba_out);
/* Device pointers on the scene's device; stream NULL = the scene's own.  Returns after the kernels complete. */
int rt_bake_irradiance_device(const RtScene* scene, uint64_t n, const double* d_positions, const double* d_normals,
                              const RtRenderParams* params, double* d_rgba_out, void* stream);
/* The points are hit records on the device (rt_trace_rays_device): pos (offset 8) and normal (offset 32) of record i, flags at
 * offset 84, 96 bytes apart.  A record without RT_RAY_HIT or with RT_RAY_ENVIRONMENT has no surface point: (0, 0, 0, 0) exactly
 * (written after the resolve; samples = n T S^2 counts such records too).  Scenes with volumes have no ray queries, so no
 * records to pass.                                                                                                      */
int rt_bake_irradiance_hits_device(const RtScene* scene, uint64_t n, const RtRayHit* d_hits, const RtRenderParams* params,
                                   double* d_rgba_out, void* stream);

/* ---- SH radiance probes ---------------------------------------------------------------------------
 * Irradiance volumes for what is not a surface of the scene - moving objects, particles, volumetric effects: the full path
 * tracer - materials, the light-biased mixture sampler, volumes, every texture - started from n positions in free space in
 * directions uniform over the sphere, and projected onto the nine real spherical harmonics of bands 0-2 on the device.
 * One fused pass: the directions are formed in registers, 24 B in and 288 B out per PROBE, no ray table, nothing stored per path.
 * positions: n x 3 doubles.  sh_out: n x 9 x 4 doubles, (r, g, b, 0) per coefficient.
 * Of `params`: sqrt_spt (S), thread_count (T), max_depth, has_background / background, light_bias, seed and precision are used;
 * R = double or float by the precision.  For probe i (its index in the whole call), replica t < T, stratum st = sy S + sx:
 *     Rng g keyed (seed, t, i, st) as a render keys (seed, replica, pixel, stratum);
 *     r1, r2 = the generator's first two uniforms - the two draws a camera spends on its jitter;
 *     u1 = (R(sx) + r1) * inv_S,  u2 = (R(sy) + r2) * inv_S              (inv_S = R(1.0 / double(S)), exactly as rt_bake_irradiance forms them)
 *     z = 1 - 2 u2,  r = sqrt(1 - z z),  phi = u1 * 2 * pi,  d = (cos(phi) r, sin(phi) r, z)       (the uniform sphere; sine and cosine
 *         from the project's deterministic sincos; no contraction; 1 - z z cannot go negative in either format, so no clamp)
 *     o = R(pos_i),  d' = (o + d) - o     (two roundings per component: what the reference's camera returns for position = o,
 *                                          first_pixel = o + d, pixel deltas 0, no aperture)
 *     the path starts at (o, d') with max_depth, on g as it now stands, with the path's usual t_min = 0.001; L is its radiance.
 *     Y_0 .. Y_8 = the real L2 basis evaluated on d (NOT on d'), in R, positive signs (no Condon-Shortley phase), the constants
 *     f64 literals rounded to R, (x, y, z) = d:
 *         Y0 = 0.28209479177387814
 *         Y1 = 0.4886025119029199 y             Y2 = 0.4886025119029199 z             Y3 = 0.4886025119029199 x
 *         Y4 = 1.0925484305920792 (x y)         Y5 = 1.0925484305920792 (y z)         Y6 = 0.31539156525252005 (3 (z z) - 1)
 *         Y7 = 1.0925484305920792 (x z)         Y8 = 0.5462742152960396 (x x - y y)
 * out[i][k] is the ordered sum a frame's pixel is: per replica the strata in order of double(Y_k) * L, each product rounded before
 * it is added, / (S^2 T), then the replicas in order; f64, no atomics.  No factor is applied on the device: out is the mean of
 * L Y_k over the sphere's samples, and the radiance coefficients are 4 pi * out.  Hence, in f64, sample (t, i, st) is the
 * reference's sample (t, pixel i, st) with that camera, and out[i] does not depend on n, the chunk size, the pool size, replica
 * grouping or tail compaction.
 * Rules, stats and the tail flag: rt_bake_irradiance's.  n = 0 is a no-op.  RT_E_INVALID with a message naming the field: a NULL
 * array, n >= 2^31, n_parts > 1, a bad precision, sqrt_spt or thread_count of 0.  RT_E_UNSUPPORTED: RT_PIPELINE_MEGAKERNEL,
 * collect_stats, max_depth = 0.  Everything is checked before the device is touched; on any error the output is untouched.
 * A scene with volumes is supported.  rt_get_stats: samples = n T S^2.  Synchronous; must not overlap a render or an update of
 * the same scene; sees the scene as rt_scene_update left it.  Probes run in chunks of RT_RAYS_CHUNK, like rays.             */
int rt_bake_probes(const RtScene* scene, uint64_t n, const double* positions, const RtRenderParams* params, double* sh_out);
/* Device pointers on the scene's device; stream NULL = the scene's own.  Returns after the kernels complete. */
int rt_bake_probes_device(const RtScene* scene, uint64_t n, const double* d_positions, const RtRenderParams* params, double* d_sh_out,
                          void* stream);
/* Lighting from probes: m queries; query j names probe[j] < n_probes of `sh` (n_probes x 9 x 4 doubles, rt_bake_probes's layout)
 * and a normal (m x 3 doubles, need not be unit length).  With w the unit normal (n / sqrt(x x + y y + z z)) and a_k = sh[probe[j]][k]:
 *     out[j] = 4 pi * ((a_0 Y0 + (2/3) * (a_1 Y1(w) + a_2 Y2(w) + a_3 Y3(w))) + (1/4) * (a_4 Y4(w) + ... + a_8 Y8(w)))
 * per channel, every sum left to right, f64 throughout (2/3 = 2.0 / 3.0), the fourth value 0: the clamped-cosine convolution of
 * the probe's radiance divided by pi - the unit of rt_bake_irradiance's output, so irradiance = pi * out.  rgba_out: m x 4 doubles.
 * m = 0 is a no-op.  RT_E_INVALID: a NULL array, m or n_probes >= 2^31, and - host variant only, checked before the device is
 * touched - an index out of range; the device variant gives (0, 0, 0, 0) for such a query.  No scene is needed: `device` is
 * the HIP device to run on.                                                                                                */
int rt_sh_irradiance(int device, const double* sh, uint64_t n_probes, const uint32_t* probe, const double* normals, uint64_t m,
                     double* rgba_out);
/* Device pointers on `device`; returns after the kernel completes. */
int rt_sh_irradiance_device(int device, const double* d_sh, uint64_t n_probes, const uint32_t* d_probe, const double* d_normals, uint64_t m,
                            double* d_rgba_out, void* stream);

/* ---- Lightmaps: a mesh's UV atlas rasterised into surface records, baked and dilated -----------
 * A width x height map over the UV square [0, 1]^2 of one mesh op: texel (x, y), x < width, y < height, has the centre
 * p = ((x + 0.5) / width, (y + 0.5) / height); no flip (row 0 is v near 0: the addressing of RT_TEX_IMAGE, so a baked map can
 * be fed back as an image texture over the mesh's own UVs) and no repeat (UVs outside the square are clipped by it).
 * For a triangle with UV corners a, b, c (the first two components of its three `uvs` entries), in f64, one rounding per
 * operation:
 *     edge(s, t, q)  = (t.u - s.u) * (q.v - s.v) - (t.v - s.v) * (q.u - s.u)
 *     cedge(s, t, q) = edge(s, t, q) if (s.u, s.v) <= (t.u, t.v) lexicographically, else -edge(t, s, q)
 *     A = cedge(a, b, c), w_a = cedge(b, c, p), w_b = cedge(c, a, p), w_c = cedge(a, b, p); if A < 0 all four are negated.
 * Two triangles that share a UV edge see exactly opposite values on it: a centre can lie in both, never in neither.  A
 * triangle covers nothing if !(A > 0) (zero area, NaN) or if it has no UV indices; otherwise it covers the texel iff
 * w_a >= 0 && w_b >= 0 && w_c >= 0.  count(x, y) = the number of the mesh's triangles that cover the texel; the texel belongs
 * to the covering triangle with the LOWEST index in RtMesh.tri_pos order.  Its record, in the order of mesh.rs:104-147:
 *     bu = w_b / A, bv = w_c / A, bw = 1 - bu - bv;   pos = v0 + (e1 * bu + e2 * bv)      (object space)
 *     normal = cross(e1, e2).to_unit() under RT_MESH_FLAT_SHADING, else n0 * bw + n1 * bu + n2 * bv
 *     every Transform above the mesh, innermost first (transform.rs:132-133): pos = M * pos, normal = (M * normal).to_unit();
 *     without any transform the normal is normalised once
 *     u, v = a * bw + b * bu + c * bv;  t = 0;  flags = RT_RAY_HIT | RT_RAY_FRONT_FACE;  material, node, prim as rt_trace_rays
 *     sets them (prim = the triangle in RtMesh.tri_pos order).
 * An uncovered texel gets the miss record (t = +inf, flags 0, ids -1, reals 0), which the _hits_device bakes skip.  Always
 * f64.  hits_out: width * height records, row-major; counts_out (may be NULL): width * height values of count(x, y).
 * `node` is the RtSceneDesc.nodes index of an RT_NODE_MESH; `instance` picks the k-th op of the compiled program that came from
 * that node (rt_scene_op_nodes), for a mesh node reached more than once.  The mesh's tables are the scene's own f64 tables
 * (built on first use), so a scene moved by rt_scene_update rasterises its new vertices.
 * The device bins the triangles into tiles of 16 x 16 texels; if the number of (triangle, tile) references exceeds
 * RT_LIGHTMAP_MAX_REFS (environment variable, read at each call, default 2^28) the call is RT_E_UNSUPPORTED with both numbers
 * in the message.  RT_E_INVALID, naming the field: a NULL array, width or height of 0 or above 16384, a node out of range or
 * not a mesh, an instance beyond the node's ops, negative passes, a bad kind.  RT_E_UNSUPPORTED: a mesh without UVs, a mesh
 * that is a volume's boundary, the reference cap, and for rt_bake_lightmap a scene with volumes and whatever the underlying
 * bake refuses.  On any error the outputs are untouched.  Synchronous; must not overlap a render or an update of the same
 * scene.  The workspace belongs to the scene, grows only and is freed by rt_scene_destroy.                                   */
int rt_lightmap_texels(const RtScene* scene, uint32_t node, uint32_t instance, uint32_t width, uint32_t height, RtRayHit* hits_out,
                       uint32_t* counts_out_or_null);
/* Device pointers on the scene's device; stream NULL = the scene's own.  Returns after the kernels complete. */
int rt_lightmap_texels_device(const RtScene* scene, uint32_t node, uint32_t instance, uint32_t width, uint32_t height, RtRayHit* d_hits_out,
                              uint32_t* d_counts_out_or_null, void* stream);
/* Host only, needs no device: the same rule by brute force (every triangle x every texel) from the description alone. */
int rt_lightmap_texels_desc(const RtSceneDesc* desc, uint32_t node, uint32_t instance, uint32_t width, uint32_t height, RtRayHit* hits_out,
                            uint32_t* counts_out_or_null);
/* Dilation: rgba = w * h * 4 doubles, coverage = w * h bytes (0 = uncovered).  In each of `passes` passes an uncovered texel
 * with at least one covered 8-neighbour takes the mean of its covered neighbours - the sum formed in the order dy = -1 .. 1,
 * dx = -1 .. 1, then divided by their number - and counts as covered (1) in the next pass; texels outside the map are not
 * neighbours; every other texel keeps its value.  passes = 0: a copy (coverage normalised to 0 / 1).  The outputs must not be
 * the inputs.  Runs on device `device`.                                                                                  */
int rt_lightmap_dilate(int device, const double* rgba, const uint8_t* coverage, uint32_t w, uint32_t h, int32_t passes, double* rgba_out,
                       uint8_t* coverage_out);
/* The same on HBM buffers of `device`, enqueued on `stream` (NULL = the null stream); returns after the kernels complete. */
int rt_lightmap_dilate_device(int device, const double* d_rgba, const uint8_t* d_coverage, uint32_t w, uint32_t h, int32_t passes,
                              double* d_rgba_out, uint8_t* d_coverage_out, void* stream);
/* A lightmap in one call, everything on the device between the stages: rt_lightmap_texels_device, then
 * rt_bake_irradiance_hits_device with render_params (kind = RT_LIGHTMAP_IRRADIANCE) or rt_bake_visibility_hits_device with
 * bake_params (kind = RT_LIGHTMAP_VISIBILITY, NULL = its defaults; visibility in r, g and b, w = 0, uncovered texels zeroed),
 * then rt_lightmap_dilate_device with dilate_passes.  rgba_out: width * height * 4 doubles; coverage_out: width * height bytes,
 * the coverage BEFORE dilation (1 = the texel has a record).                                                              */
#define RT_LIGHTMAP_IRRADIANCE 0u
#define RT_LIGHTMAP_VISIBILITY 1u
int rt_bake_lightmap(const RtScene* scene, uint32_t node, uint32_t instance, uint32_t width, uint32_t height, uint32_t kind,
                     const RtRenderParams* render_params, const RtBakeParams* bake_params, int32_t dilate_passes, double* rgba_out,
                     uint8_t* coverage_out);
int rt_bake_lightmap_device(const RtScene* scene, uint32_t node, uint32_t instance, uint32_t width, uint32_t height, uint32_t kind,
                            const RtRenderParams* render_params, const RtBakeParams* bake_params, int32_t dilate_passes, double* d_rgba_out,
                            uint8_t* d_coverage_out, void* stream);
/* Of the last rasterisation on this scene (rt_lightmap_texels* and rt_bake_lightmap*). */
typedef struct RtLightmapStats {
    double   bin_ms;             /* HIP-event time of the per-tile counts, the scan and the fill */
    double   raster_ms;          /* HIP-event time of the raster kernel */
    uint64_t texels;             /* width * height */
    uint64_t covered_texels;
    uint64_t tile_refs;          /* (triangle, tile) references */
    uint32_t width, height;
    uint32_t _reserved[4];
} RtLightmapStats;
int rt_lightmap_stats(const RtScene* scene, RtLightmapStats* out);

/* Message for the last non-RT_OK status on this thread ("" if none). */
const char* rt_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355_H */
