// drt/hip.hpp -- host glue above the C ABI (include/drt_hip.h): the batched, device-side
// replacement of the reference's pixel x sample loop (src/render.cpp:72-86).
//
//   drt::hip::render(scene, cam, tracer, spp, img [, options [, adjoint]])
//
// walks a drt::Scene<T> through the additive describe()/kind()/parameter() hooks, deduplicates the
// scene parameters by tape-node identity (handles share nodes: `white` feeds two materials in
// render.cpp:28,34-35), uploads the POD scene, renders on one or several MI355X devices and, when
// options.backward is set, ADDS the returned gradients into param.grad() -- the accumulate
// semantics of VariableNode::backward (vector.hpp:185-188).  Several devices = ONE group context
// (drt_hip_create_group): the library deals the row bands to the devices, runs them side by side and
// sums the gradient vector across them with a single RCCL all-reduce; this header adds nothing.
//
//   drt::hip::render_tangent(scene, cam, tracer, spp, {{param, direction}, ...}, img, tangent_img [, options])
//   drt::hip::render_tangents(scene, cam, tracer, spp, {direction, ...}, img, tangent_imgs [, options])      up to 8 directions, one render
//   drt::hip::render_param_sets(scene, cam, tracer, spp, {set, ...}, target, imgs, &losses [, options])      up to 8 parameter sets, one trace
//   drt::hip::render_param_sets_along(scene, cam, tracer, spp, {set, ...}, target [, imgs, tangent_imgs, options])   up to 4 sets with a direction each: loss, slope, curvature
//   drt::hip::render_param_sets_grad(scene, cam, tracer, spp, {set, ...} [, adjoints, options])     up to 8 sets with a summed gradient each, one trace
//   drt::hip::render_views(scene, {cam, ...}, tracer, spp, imgs [, options, adjoints, seeds])       up to 64 cameras of one size, one trace
//   drt::hip::render_pixels(scene, {cam, ...}, {{pixel, ...}, ...}, tracer, spp, out [, options, adjoints, seeds])   a batch of pixels of up to 64 cameras, one trace
//   drt::hip::normal_equations_along(scene, cam, tracer, spp, {direction, ...}, options, target_or_residual) Gauss-Newton in their span
//   drt::hip::normal_equations_cross(scene, cam, tracer, spp, {direction, ...}, options, target)             ... unbiased from one render
//   drt::hip::render(scene of Dual<U>, ...)
//
// forward mode (drt_hip_render_tangent): the image and its derivative along one direction of parameter space -- given as
// (handle, direction) pairs, or as the dual parts of a Scene<Dual<U>>'s parameters, the reference's own validation run
// (dual.hpp) on the device.
//
// No CPU fallback: if libdrt_hip.so cannot create a context this throws std::runtime_error.
#pragma once

#include <cstdint>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../drt_hip.h"
#include "camera.hpp"
#include "dual.hpp"
#include "mesh.hpp"
#include "pathtracer.hpp"

namespace drt { namespace hip {

struct Options {
    bool backward = false;          // also back-propagate (render.cpp:80, commented out there)
    bool unbiased = false;          // backward with the unbiased integration operator (integrate.hpp:39-52)
    bool sample_loss_l2 = false;    // `adjoint` is a TARGET image: every sample is back-propagated through a loss of its own,
                                    // |radiance - target|^2 (README.md:93-98 with loss_func = squared error; DRT_RENDER_LOSS_L2)
    uint32_t seed = 1;
    int max_depth = 0;              // 0 = library default (64)
    std::vector<int> devices = {0}; // pixel-row bands are dealt round-robin to these devices (several: one group
                                    // context, gradients reduced across them by RCCL inside the library)
    int band_rows = 16;
    bool f64 = false;               // verification mode: compute in double on the device
    long long batch_paths = 0;
    int bounces_per_launch = 0;     // 0 = automatic; 1 = one shade launch per bounce (drt_hip.h)
    bool reuse_context = true;      // keep the device context (and its gigabytes of queues) between calls
};

struct Stats {
    unsigned long long paths = 0, segments = 0;
    unsigned long long capped_paths = 0;   // paths Options::max_depth cut short (the reference has no cap)
    double ms = 0;
};

template <typename T>
struct FlatScene {
    std::vector<drt_shape_desc> shapes;
    std::vector<drt_material_desc> materials;
    std::vector<drt_emitter_desc> emitters;
    std::vector<double> params;
    std::vector<uint8_t> requires_grad;
    std::vector<Vector<T, 3, true>> handles;   // one per parameter, sharing the user's nodes
    std::vector<drt_mesh_desc> meshes;
    std::vector<std::vector<double>> mesh_vertices;
    std::vector<std::vector<uint32_t>> mesh_indices;
    std::vector<drt_shape_kind_desc> kinds;    // caller-defined shape kinds (ShapeKind::User), by kind_name
    std::vector<double> user_params;           // n_shapes x 4: values 4..7 of the shapes' records
    std::vector<drt_bxdf_kind_desc> bxdf_kinds;   // caller-defined BxDF kinds (BxDFKind::User), by name
    std::vector<double> user_bxdf_params;      // n_materials: value 1 of the materials' records

    drt_scene_desc desc() const
    {
        drt_scene_desc d;
        d.n_shapes = (int32_t)shapes.size();
        d.n_materials = (int32_t)materials.size();
        d.n_emitters = (int32_t)emitters.size();
        d.n_params = (int32_t)requires_grad.size();
        d.shapes = shapes.data();
        d.materials = materials.data();
        d.emitters = emitters.data();
        d.params = params.data();
        d.requires_grad = requires_grad.data();
        d.n_meshes = (int32_t)meshes.size();
        d.n_kinds = kinds.empty() ? (bxdf_kinds.empty() ? 0 : -1) : (int32_t)kinds.size();
        d.meshes = meshes.data();
        d.kinds = kinds.data();
        d.user_params = kinds.empty() ? nullptr : user_params.data();
        d.n_bxdf_kinds = (int32_t)bxdf_kinds.size();
        d.reserved2 = 0;
        d.bxdf_kinds = bxdf_kinds.data();
        d.user_bxdf_params = bxdf_kinds.empty() ? nullptr : user_bxdf_params.data();
        return d;
    }

    // Everything but the parameter VALUES (FNV-1a over the records and the mesh data): two scenes with the
    // same key differ at most in their parameters, which drt_hip_update_params replaces without
    // re-uploading the geometry or rebuilding the BVH.
    uint64_t topology_key() const
    {
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](const void* p, std::size_t n) {
            const unsigned char* b = static_cast<const unsigned char*>(p);
            for (std::size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
        };
        auto mix_n = [&](uint64_t v) { mix(&v, sizeof v); };
        mix_n(shapes.size());
        for (const drt_shape_desc& sh : shapes) {       // field by field: the records have padding
            mix(&sh.type, sizeof sh.type); mix(&sh.material, sizeof sh.material); mix(&sh.emitter, sizeof sh.emitter);
            mix(&sh.mesh, sizeof sh.mesh); mix(sh.p, sizeof sh.p);
        }
        mix_n(kinds.size());
        for (const drt_shape_kind_desc& k : kinds) {
            mix(k.intersect_src, std::strlen(k.intersect_src));
            mix(k.normal_src, std::strlen(k.normal_src));
        }
        if (!kinds.empty())
            mix(user_params.data(), user_params.size() * sizeof(double));
        mix_n(bxdf_kinds.size());
        for (const drt_bxdf_kind_desc& k : bxdf_kinds)
            mix(k.sample_src, std::strlen(k.sample_src));
        if (!bxdf_kinds.empty())
            mix(user_bxdf_params.data(), user_bxdf_params.size() * sizeof(double));
        mix_n(materials.size());
        for (const drt_material_desc& m : materials) {
            mix(&m.type, sizeof m.type); mix(&m.param, sizeof m.param); mix(&m.exponent, sizeof m.exponent);
        }
        mix_n(emitters.size());
        for (const drt_emitter_desc& e : emitters)
            mix(&e.param, sizeof e.param);
        mix_n(requires_grad.size());
        mix(requires_grad.data(), requires_grad.size());
        mix_n(meshes.size());
        for (std::size_t i = 0; i < meshes.size(); ++i) {
            mix(mesh_vertices[i].data(), mesh_vertices[i].size() * sizeof(double));
            mix(mesh_indices[i].data(), mesh_indices[i].size() * sizeof(uint32_t));
            mix_n(meshes[i].face_material ? 1 : 0);
            if (meshes[i].face_material)
                mix(meshes[i].face_material, (std::size_t)meshes[i].n_triangles * sizeof(int32_t));
        }
        return h;
    }
};

template <typename T>
inline FlatScene<T> flatten(const Scene<T>& scene)
{
    FlatScene<T> f;
    std::map<const void*, int> param_of, material_of, emitter_of;
    auto param_index = [&](const Vector<T, 3, true>& h) {
        auto it = param_of.find(h.id());
        if (it != param_of.end())
            return it->second;
        const int idx = (int)f.handles.size();
        param_of[h.id()] = idx;
        f.handles.push_back(h);
        for (int c = 0; c < 3; ++c)
            f.params.push_back(double(real(h[c])));
        f.requires_grad.push_back(h.requires_grad() ? 1 : 0);
        return idx;
    };
    for (Shape<T>* shape : scene) {
        const ShapeRecord rec = shape->describe();
        drt_shape_desc sd{};
        if (rec.kind == ShapeKind::Plane)
            sd.type = DRT_SHAPE_PLANE;
        else if (rec.kind == ShapeKind::Sphere)
            sd.type = DRT_SHAPE_SPHERE;
        else if (rec.kind == ShapeKind::Mesh) {
            auto* mesh = dynamic_cast<Mesh<T>*>(shape);
            if (!mesh)
                throw std::runtime_error("drt::hip: ShapeKind::Mesh reported by a shape that is not drt::Mesh");
            sd.type = DRT_SHAPE_MESH;
            sd.mesh = (int32_t)f.mesh_vertices.size();
            std::vector<double> vs;
            for (const auto& v : mesh->vertices())
                for (int c = 0; c < 3; ++c)
                    vs.push_back(double(real(v[c])));
            std::vector<uint32_t> is;
            for (const auto& t : mesh->triangles())
                for (int c = 0; c < 3; ++c)
                    is.push_back(t[c]);
            f.mesh_vertices.push_back(std::move(vs));
            f.mesh_indices.push_back(std::move(is));
        } else if (rec.kind == ShapeKind::User) {
            // any other analytic shape: its own intersect / normal, compiled into the scene's path kernel (ABI v8)
            if (!rec.kind_name || !rec.intersect_src || !rec.normal_src)
                throw std::runtime_error("drt::hip: a ShapeKind::User record needs kind_name, intersect_src and normal_src");
            int k = -1;
            for (std::size_t i = 0; i < f.kinds.size(); ++i)
                if (std::strcmp(f.kinds[i].name, rec.kind_name) == 0)
                    k = (int)i;
            if (k < 0) {
                if (f.kinds.size() >= DRT_MAX_USER_KINDS)
                    throw std::runtime_error("drt::hip: more caller-defined shape kinds in one scene than the device path takes (DRT_MAX_USER_KINDS)");
                drt_shape_kind_desc kd{rec.kind_name, rec.intersect_src, rec.normal_src};
                k = (int)f.kinds.size();
                f.kinds.push_back(kd);
            }
            sd.type = DRT_SHAPE_USER;
            sd.mesh = k;
        } else
            throw std::runtime_error("drt::hip: shape type has no device record (describe() reports neither one of the library's kinds "
                                     "nor ShapeKind::User with its source)");
        for (int i = 0; i < 4; ++i)
            sd.p[i] = rec.p[i];
        for (int i = 0; i < 4; ++i)
            f.user_params.push_back(rec.q[i]);
        sd.material = -1;
        sd.emitter = -1;
        if (BxDF<T>* b = shape->bxdf()) {
            auto it = material_of.find(b);
            if (it == material_of.end()) {
                drt_material_desc md{};
                if (b->kind() == BxDFKind::Diffuse)
                    md.type = DRT_BXDF_DIFFUSE;
                else if (b->kind() == BxDFKind::Specular)
                    md.type = DRT_BXDF_SPECULAR;
                else if (b->kind() == BxDFKind::Mirror)
                    md.type = DRT_BXDF_MIRROR;
                else if (b->kind() == BxDFKind::User) {
                    // any other BxDF of the form colour x scalar: its own sample-and-evaluate body, compiled into the scene's path kernel
                    if (!b->device_kind_name() || !b->device_sample_src() || !b->parameter())
                        throw std::runtime_error("drt::hip: a BxDFKind::User material needs device_kind_name(), device_sample_src() and parameter()");
                    int k = -1;
                    for (std::size_t i = 0; i < f.bxdf_kinds.size(); ++i)
                        if (std::strcmp(f.bxdf_kinds[i].name, b->device_kind_name()) == 0)
                            k = (int)i;
                    if (k < 0) {
                        if (f.bxdf_kinds.size() >= DRT_MAX_USER_BXDF_KINDS)
                            throw std::runtime_error("drt::hip: more caller-defined BxDF kinds in one scene than the device path takes (DRT_MAX_USER_BXDF_KINDS)");
                        drt_bxdf_kind_desc kd{b->device_kind_name(), b->device_sample_src()};
                        k = (int)f.bxdf_kinds.size();
                        f.bxdf_kinds.push_back(kd);
                    }
                    md.type = DRT_BXDF_USER + k;
                } else
                    throw std::runtime_error("drt::hip: BxDF type has no device record (kind() reports neither one of the library's kinds "
                                             "nor BxDFKind::User with its source)");
                md.param = md.type == DRT_BXDF_MIRROR ? -1 : param_index(*b->parameter());
                md.exponent = b->exponent();
                it = material_of.emplace(b, (int)f.materials.size()).first;
                f.materials.push_back(md);
                f.user_bxdf_params.push_back(b->value1());
            }
            sd.material = it->second;
        }
        if (Emitter<T>* e = shape->emitter()) {
            auto it = emitter_of.find(e);
            if (it == emitter_of.end()) {
                auto* area = dynamic_cast<AreaEmitter<T>*>(e);
                if (!area)
                    throw std::runtime_error("drt::hip: emitter type has no device record");
                drt_emitter_desc ed{};
                ed.param = param_index(area->parameter());
                it = emitter_of.emplace(e, (int)f.emitters.size()).first;
                f.emitters.push_back(ed);
            }
            sd.emitter = it->second;
        }
        f.shapes.push_back(sd);
    }
    for (std::size_t m = 0; m < f.mesh_vertices.size(); ++m) {   // pointers taken once the vectors stopped growing
        drt_mesh_desc md{};
        md.n_vertices = (int32_t)(f.mesh_vertices[m].size() / 3);
        md.n_triangles = (int32_t)(f.mesh_indices[m].size() / 3);
        md.vertices = f.mesh_vertices[m].data();
        md.indices = f.mesh_indices[m].data();
        md.face_material = nullptr;
        md.face_param = nullptr;
        f.meshes.push_back(md);
    }
    return f;
}

template <typename T>
inline drt_camera_desc describe(const Camera<T>& cam)
{
    drt_camera_desc c{};
    c.width = (int32_t)cam.width();
    c.height = (int32_t)cam.height();
    c.vfov = cam.vfov();
    for (int i = 0; i < 3; ++i) {
        c.eye[i] = double(real(cam.eye()[i]));
        c.forward[i] = double(real(cam.forward()[i]));
        c.right[i] = double(real(cam.right()[i]));
        c.up[i] = double(real(cam.up()[i]));
    }
    return c;
}

class Context {
public:
    explicit Context(int device) : Context(std::vector<int>{device}) {}
    // one device: a plain context; several: a group context (the library owns the RCCL communicators)
    explicit Context(const std::vector<int>& devices)
    {
        if (devices.empty())
            throw std::runtime_error("drt::hip::Context: no device given");
        const int rc = devices.size() == 1 ? drt_hip_create(devices[0], &m_ctx)
                                           : drt_hip_create_group(devices.data(), (int)devices.size(), &m_ctx);
        if (rc != DRT_OK) {
            std::string list;
            for (int d : devices)
                list += (list.empty() ? "" : ", ") + std::to_string(d);
            throw std::runtime_error("drt_hip_create" + std::string(devices.size() == 1 ? "" : "_group") + "(device " + list +
                                     ") failed with status " + std::to_string(rc) + " (no HIP device? there is no CPU fallback)");
        }
    }
    ~Context() { drt_hip_destroy(m_ctx); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    drt_hip_ctx* get() const { return m_ctx; }
    void check(int rc, const char* what) const
    {
        if (rc != DRT_OK)
            throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " + drt_hip_last_error(m_ctx));
    }
    std::mutex& mutex() { return m_mutex; }

    // upload the scene, or -- when only parameter values changed since this context's last upload -- just them
    template <typename T>
    void set_scene(const FlatScene<T>& flat)
    {
        const uint64_t key = flat.topology_key();
        if (m_has_scene && key == m_scene_key) {
            if (flat.params == m_params)       // nothing changed (drt_hip_update_params waits for the frames in flight)
                return;
            check(drt_hip_update_params(m_ctx, flat.params.data()), "drt_hip_update_params");
            m_params = flat.params;
            return;
        }
        const drt_scene_desc sd = flat.desc();
        m_has_scene = false;
        check(drt_hip_upload_scene(m_ctx, &sd), "drt_hip_upload_scene");
        m_scene_key = key;
        m_params = flat.params;
        m_has_scene = true;
    }

    // host buffers of the (at most DRT_HIP_FRAMES_IN_FLIGHT) frames in flight: kept, so that a frame costs no 3 MB allocation
    std::vector<float> frame_pool[DRT_HIP_FRAMES_IN_FLIGHT];
    std::vector<double> grad_pool[DRT_HIP_FRAMES_IN_FLIGHT];
    bool slot_in_flight[DRT_HIP_FRAMES_IN_FLIGHT] = {};   // the slot's buffers belong to a frame that has not been collected
    unsigned submitted = 0;
    // The frame buffer of the SYNCHRONOUS call, kept between calls and -- on a plain context -- pinned (drt_hip_pin_host): the
    // device's finishing kernel then writes a frame straight into it; no 3 MB allocation, staging copy or memcpy per call.
    float* sync_frame(std::size_t n_floats, bool plain)
    {
        if (m_sync_frame.size() != n_floats) {
            if (m_sync_pinned) {
                (void)drt_hip_unpin_host(m_ctx, m_sync_frame.data());
                m_sync_pinned = false;
            }
            m_sync_frame.assign(n_floats, 0.f);
            if (plain && n_floats)
                m_sync_pinned = drt_hip_pin_host(m_ctx, m_sync_frame.data(), n_floats * sizeof(float)) == DRT_OK;
        }
        return m_sync_frame.data();
    }

private:
    drt_hip_ctx* m_ctx = nullptr;
    uint64_t m_scene_key = 0;
    std::vector<double> m_params;      // the parameter values the device holds
    std::vector<float> m_sync_frame;
    bool m_sync_pinned = false;
    bool m_has_scene = false;
    std::mutex m_mutex;        // a context is not thread-safe: pooled ones are locked for the duration of a call
};

// Contexts are kept between calls: creating one (HIP module load, stream) and growing its queues
// (gigabytes of hipMalloc for a 512 x 512 x 64 frame) costs ~0.3 s, a render 2 ms -- an optimisation
// loop around drt::hip::render must not pay that per iteration.  One context per device list (a
// group context for several devices).  They live until release_contexts() or process exit
// (deliberately not destroyed by static destructors: the HIP runtime may be gone by then).
namespace detail {
struct ContextPool {
    std::mutex m;
    std::map<std::vector<int>, Context*> contexts;
};
inline ContextPool& pool()
{
    static ContextPool* p = new ContextPool();
    return *p;
}
} // namespace detail

inline Context& pooled_context(const std::vector<int>& devices)
{
    detail::ContextPool& p = detail::pool();
    std::lock_guard<std::mutex> lock(p.m);
    Context*& c = p.contexts[devices];
    if (!c)
        c = new Context(devices);
    return *c;
}
inline Context& pooled_context(int device) { return pooled_context(std::vector<int>{device}); }

inline void release_contexts()
{
    detail::ContextPool& p = detail::pool();
    std::lock_guard<std::mutex> lock(p.m);
    for (auto& kv : p.contexts)
        delete kv.second;
    p.contexts.clear();
}

// ---- what the entry points below share ------------------------------------------------------------------------------
namespace detail {
// THE place a drt_render_params is filled.  Every entry point renders whole frames: n_shards = 1 (the library reads band_rows
// only where it deals bands out -- a group context to its devices -- and normalises n_shards <= 1 to 1: csrc/drt_render.h).
inline drt_render_params render_params(double absorb, std::size_t min_bounces, std::size_t spp, const Options& opt, uint32_t flags)
{
    drt_render_params rp{};
    rp.spp = (int32_t)spp;
    rp.min_bounces = (int32_t)min_bounces;
    rp.absorb = absorb;
    rp.max_depth = opt.max_depth;
    rp.seed = opt.seed;
    rp.shard = 0;
    rp.n_shards = 1;
    rp.band_rows = opt.band_rows;
    rp.flags = flags;
    rp.batch_paths = opt.batch_paths;
    rp.bounces_per_launch = opt.bounces_per_launch;
    return rp;
}
inline uint32_t f64_flag(const Options& opt) { return opt.f64 ? DRT_RENDER_F64 : 0u; }
// render / submit: the operator and the per-sample loss are notions of the backward pass
inline uint32_t reverse_flags(const Options& opt)
{
    return f64_flag(opt) | (opt.backward ? DRT_RENDER_BACKWARD : 0u) | (opt.backward && opt.unbiased ? DRT_RENDER_UNBIASED : 0u) |
           (opt.backward && opt.sample_loss_l2 ? DRT_RENDER_LOSS_L2 : 0u);
}
inline Stats to_stats(const drt_hip_stats& st)
{
    Stats out;
    out.paths = st.paths;
    out.segments = st.segments;
    out.capped_paths = st.capped_paths;
    out.ms = st.ms_total;
    return out;
}

// A context for the duration of one call -- the call's own (Options::reuse_context off: destroyed with the session) or the pooled
// one of its devices --, locked, holding the scene.
struct Session {
    std::unique_ptr<Context> own;
    Context& ctx;
    std::lock_guard<std::mutex> lock;
    // render: every device of opt.devices (several: one group context)
    template <typename T>
    static Session on_all_devices(const Options& opt, const FlatScene<T>& flat) { return Session(opt.devices, opt.reuse_context, flat); }
    // the single-device entry points: the first device listed, device 0 where none is
    template <typename T>
    static Session on_first_device(const Options& opt, const FlatScene<T>& flat)
    {
        return Session(std::vector<int>{opt.devices.empty() ? 0 : opt.devices[0]}, opt.reuse_context, flat);
    }

private:
    template <typename T>
    Session(const std::vector<int>& devices, bool reuse_context, const FlatScene<T>& flat)
        : own(reuse_context ? nullptr : new Context(devices)), ctx(own ? *own : pooled_context(devices)), lock(ctx.mutex())
    {
        ctx.set_scene(flat);
    }
};

// width x height pixels <-> the library's buffers of 3 values per pixel
template <typename T>
inline std::vector<float> to_floats(const Vector<T, 3>* src, std::size_t npix)
{
    std::vector<float> out(npix * 3);
    for (std::size_t i = 0; i < npix; ++i)
        for (int c = 0; c < 3; ++c)
            out[i * 3 + c] = float(real(src[i][c]));
    return out;
}
template <typename F, typename T>
inline void from_buffer(const F* src, std::size_t npix, Vector<T, 3>* dst)
{
    if (!dst)
        return;
    for (std::size_t i = 0; i < npix; ++i)
        for (int c = 0; c < 3; ++c)
            dst[i][c] = T(src[i * 3 + c]);
}

// the returned gradients ADDED to the parameters that take one, like m_grad += grad (vector.hpp:185-188)
template <typename T>
inline void accumulate_grads(std::vector<Vector<T, 3, true>>& handles, const std::vector<uint8_t>& requires_grad, const double* grads)
{
    for (std::size_t p = 0; p < handles.size(); ++p) {
        if (!requires_grad[p])
            continue;
        Vector<T, 3> g(T(0));
        for (int c = 0; c < 3; ++c)
            g[c] = T(grads[p * 3 + c]);
        handles[p].grad() += g;
    }
}

// the scene's parameter that shares `handle`'s node
template <typename T>
inline int param_index(const FlatScene<T>& flat, const Vector<T, 3, true>& handle, const char* message_if_unused)
{
    for (std::size_t p = 0; p < flat.handles.size(); ++p)
        if (flat.handles[p].id() == handle.id())
            return (int)p;
    throw std::runtime_error(message_if_unused);
}

// what the forward-mode entry points refuse before they flatten the scene, in the caller's words (`what`: "forward mode", "a forward render")
inline void forward_only(const char* who, const Options& opt, const char* what)
{
    if (opt.backward || opt.unbiased || opt.sample_loss_l2)
        throw std::runtime_error(std::string(who) + ": " + what + " takes no reverse-mode option (backward, unbiased, sample_loss_l2)");
}
inline void one_device(const char* who, const Options& opt)
{
    if (opt.devices.size() > 1)
        throw std::runtime_error(std::string(who) + ": one device (render shards on plain contexts and add them)");
}

// K x n_params x 3 rows as the ABI takes them, from K lists of entries that name a handle and a value (entry(t) -> their addresses): every
// row starts as `start` (n_params x 3; nullptr: zeros) and takes each listed value at its handle's place.  `add`: a handle listed twice
// adds up -- what render_tangent documents for DIRECTIONS, and only they do it; a set's values and directions keep the last one listed
template <typename T, typename List, typename Entry>
inline std::vector<double> rows_of(const char* who, const FlatScene<T>& flat, const std::vector<List>& lists, const double* start, bool add, Entry entry)
{
    const std::size_t n = flat.handles.size() * 3;
    const std::string unused = std::string(who) + ": a listed parameter is not used by the scene";
    std::vector<double> v(lists.size() * n, 0.0);
    for (std::size_t k = 0; k < lists.size(); ++k) {
        if (start)
            std::copy(start, start + n, v.begin() + (std::ptrdiff_t)(k * n));
        for (const auto& t : lists[k]) {
            const std::pair<const Vector<T, 3, true>*, const Vector<T, 3>*> e = entry(t);
            const int index = param_index(flat, *e.first, unused.c_str());
            for (int c = 0; c < 3; ++c) {
                double& at = v[k * n + (std::size_t)index * 3 + c];
                const double value = double(real((*e.second)[c]));
                at = add ? at + value : value;
            }
        }
    }
    return v;
}

// One channel's Levenberg-Marquardt step: (A + lambda diag A) x = -b over the chosen `rows` of the P x P matrix A (row-major), by a
// Cholesky factorisation.  -> x, x[i] for rows[i].  Throws `not_positive_definite` where the damped matrix is not.
inline std::vector<double> damped_cholesky(const double* A, const double* b, std::size_t P, const std::vector<std::size_t>& rows, double lambda,
                                           const char* not_positive_definite)
{
    const std::size_t n = rows.size();
    std::vector<double> L(n * n), y(n), x(n);
    // M = A + lambda diag A = L L^T (lower triangle, row by row)
    for (std::size_t i = 0; i < n; ++i)
        for (std::size_t j = 0; j <= i; ++j) {
            double v = A[rows[i] * P + rows[j]] * (i == j ? 1.0 + lambda : 1.0);
            for (std::size_t k = 0; k < j; ++k)
                v -= L[i * n + k] * L[j * n + k];
            if (i == j) {
                if (!(v > 0.0))
                    throw std::runtime_error(not_positive_definite);
                L[i * n + i] = std::sqrt(v);
            } else
                L[i * n + j] = v / L[j * n + j];
        }
    for (std::size_t i = 0; i < n; ++i) {          // L y = -b
        double v = -b[rows[i]];
        for (std::size_t k = 0; k < i; ++k)
            v -= L[i * n + k] * y[k];
        y[i] = v / L[i * n + i];
    }
    for (std::size_t ii = n; ii-- > 0;) {           // L^T x = y
        double v = y[ii];
        for (std::size_t k = ii + 1; k < n; ++k)
            v -= L[k * n + ii] * x[k];
        x[ii] = v / L[ii * n + ii];
    }
    return x;
}
} // namespace detail

// img: width*height row-major (render.cpp:66,82); adjoint: optional per-pixel seed, same layout.
template <typename T>
inline Stats render(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                    Vector<T, 3>* img, const Options& opt = Options(), const Vector<T, 3>* adjoint = nullptr)
{
    FlatScene<T> flat = flatten(scene);
    const drt_camera_desc cd = describe(cam);
    const std::size_t npix = cam.width() * cam.height();
    if (opt.devices.empty())
        throw std::runtime_error("drt::hip::render: no device given");
    const std::vector<float> adj = adjoint ? detail::to_floats(adjoint, npix) : std::vector<float>();
    const drt_render_params rp = detail::render_params(tracer.absorb(), tracer.min_bounces(), spp, opt, detail::reverse_flags(opt));
    std::vector<double> grads(flat.requires_grad.size() * 3, 0.0);
    drt_hip_stats st{};
    {
        detail::Session s = detail::Session::on_all_devices(opt, flat);
        // the frame: a buffer of this call's beside a context of its own, else the pooled context's (pinned on a plain context)
        std::vector<float> own_frame(s.own ? npix * 3 : 0, 0.f);
        float* frame = s.own ? own_frame.data() : s.ctx.sync_frame(npix * 3, opt.devices.size() == 1);
        // several devices: out_param_grad comes back ALREADY summed over them (one ncclAllReduce in the library)
        s.ctx.check(drt_hip_render(s.ctx.get(), &cd, &rp, adjoint ? adj.data() : nullptr, frame, opt.backward ? grads.data() : nullptr, &st),
                    "drt_hip_render");
        detail::from_buffer(frame, npix, img);                 // (under the context's lock: the buffer is the context's)
    }
    if (opt.backward)
        detail::accumulate_grads(flat.handles, flat.requires_grad, grads.data());
    return detail::to_stats(st);
}

// ---- frames in flight ----------------------------------------------------------------------------------
// render() returns with the frame in `img`: a device-to-host copy and a wait per call, the GPU idle meanwhile.  A loop
// that renders frame after frame (several views or mini-batches per optimisation step, a turntable) submits the next
// frame before it collects the previous one:
//     auto a = drt::hip::submit(scene, cam, tracer, spp, img_a, opt);
//     auto b = drt::hip::submit(scene, cam, tracer, spp, img_b, opt);   // at most four in flight per device context
//     a.get();  b.get();             // img_* filled, gradients ADDED into param.grad() (vector.hpp:185-188) at get()
// (drt_hip_render_async / drt_hip_wait: frame i's results travel to a pinned block while frame i + 1's kernels run.)
// One device (opt.devices[0]); the frames of one context belong to one thread; the scene's geometry must not change
// between submit and get (parameter values may: a submit uploads them).
template <typename T>
class Pending {
public:
    Pending() = default;
    Pending(Pending&& o) noexcept { *this = std::move(o); }
    // A frame that is dropped without get() -- an exception between submit and get, a handle that is overwritten -- is still
    // waited for and its results discarded: its slot of the (process-wide, pooled) context would otherwise stay in flight for
    // ever and every later render on that device would be refused.
    ~Pending() { discard(); }
    Pending& operator=(Pending&& o) noexcept
    {
        if (this == &o)
            return *this;
        discard();
        m_ctx = o.m_ctx; o.m_ctx = nullptr;            // (the source no longer owns a frame)
        m_slot = o.m_slot;
        m_ticket = o.m_ticket; m_img = o.m_img; m_backward = o.m_backward;
        m_frame = o.m_frame; m_grads = o.m_grads; m_npix = o.m_npix;
        m_requires_grad = std::move(o.m_requires_grad); m_handles = std::move(o.m_handles);
        return *this;
    }
    Pending(const Pending&) = delete;
    Pending& operator=(const Pending&) = delete;
    bool valid() const { return m_ctx != nullptr; }
    // wait for the frame, hand it over, accumulate its gradients
    Stats get()
    {
        if (!m_ctx)
            throw std::runtime_error("drt::hip::Pending::get: no frame");
        drt_hip_stats st{};
        Context* ctx = m_ctx;
        m_ctx = nullptr;
        std::lock_guard<std::mutex> lock(ctx->mutex());
        const int rc = drt_hip_wait(ctx->get(), m_ticket, &st);
        ctx->slot_in_flight[m_slot] = false;
        ctx->check(rc, "drt_hip_wait");
        detail::from_buffer(m_frame, m_npix, m_img);
        if (m_backward)
            detail::accumulate_grads(m_handles, m_requires_grad, m_grads);
        return detail::to_stats(st);
    }

private:
    void discard() noexcept
    {
        if (!m_ctx)
            return;
        Context* ctx = m_ctx;
        m_ctx = nullptr;
        std::lock_guard<std::mutex> lock(ctx->mutex());
        (void)drt_hip_wait(ctx->get(), m_ticket, nullptr);      // (into the pool's buffers; nothing is accumulated)
        ctx->slot_in_flight[m_slot] = false;
    }
    template <typename U>
    friend Pending<U> submit(const Scene<U>&, const Camera<U>&, const Pathtracer<U>&, std::size_t, Vector<U, 3>*, const Options&,
                             const Vector<U, 3>*);
    Context* m_ctx = nullptr;
    unsigned m_slot = 0;
    uint64_t m_ticket = 0;
    Vector<T, 3>* m_img = nullptr;
    bool m_backward = false;
    float* m_frame = nullptr;                   // written by drt_hip_wait: buffers of the context's pool (a set per frame in flight)
    double* m_grads = nullptr;
    std::size_t m_npix = 0;
    std::vector<uint8_t> m_requires_grad;
    std::vector<Vector<T, 3, true>> m_handles;
};

template <typename T>
inline Pending<T> submit(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                         Vector<T, 3>* img, const Options& opt = Options(), const Vector<T, 3>* adjoint = nullptr)
{
    if (opt.devices.size() != 1)
        throw std::runtime_error("drt::hip::submit: one device (frames in flight are per device context)");
    FlatScene<T> flat = flatten(scene);
    const drt_camera_desc cd = describe(cam);
    const std::size_t npix = cam.width() * cam.height();
    const std::vector<float> adj = adjoint ? detail::to_floats(adjoint, npix) : std::vector<float>();
    Pending<T> f;
    f.m_img = img;
    f.m_backward = opt.backward;
    f.m_requires_grad = flat.requires_grad;
    f.m_handles = flat.handles;
    Context& ctx = pooled_context(opt.devices);
    std::lock_guard<std::mutex> lock(ctx.mutex());
    const unsigned slot = ctx.submitted % DRT_HIP_FRAMES_IN_FLIGHT;
    // (before the slot's buffers are touched: a frame still in flight is written into them at its get())
    if (ctx.slot_in_flight[slot])
        throw std::runtime_error("drt::hip::submit: four frames are in flight on this device -- get() the oldest one first");
    if (ctx.frame_pool[slot].size() < npix * 3) ctx.frame_pool[slot].resize(npix * 3);
    if (ctx.grad_pool[slot].size() < flat.requires_grad.size() * 3) ctx.grad_pool[slot].resize(flat.requires_grad.size() * 3);
    f.m_frame = ctx.frame_pool[slot].data();
    f.m_grads = ctx.grad_pool[slot].data();
    f.m_npix = npix;
    ctx.set_scene(flat);
    const drt_render_params rp = detail::render_params(tracer.absorb(), tracer.min_bounces(), spp, opt, detail::reverse_flags(opt));
    ctx.check(drt_hip_render_async(ctx.get(), &cd, &rp, adjoint ? adj.data() : nullptr, f.m_frame,
                                   opt.backward ? f.m_grads : nullptr, &f.m_ticket),
              "drt_hip_render_async");
    ++ctx.submitted;
    ctx.slot_in_flight[slot] = true;
    f.m_slot = slot;
    f.m_ctx = &ctx;
    return f;
}

// Per-pixel gradient image of ONE parameter (the figure of the reference's README.md:142-145):
// gimg[pixel] = mean over the pixel's samples of d(seed . radiance)/d param.  Single device.
template <typename T>
inline Stats render_gradient_image(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer,
                                   std::size_t spp, const Vector<T, 3, true>& param, Vector<T, 3>* img,
                                   Vector<T, 3>* gimg, const Options& opt = Options())
{
    FlatScene<T> flat = flatten(scene);
    const int index = detail::param_index(flat, param, "drt::hip::render_gradient_image: the parameter is not used by the scene");
    const drt_camera_desc cd = describe(cam);
    const std::size_t npix = cam.width() * cam.height();
    std::vector<float> rgb(npix * 3, 0.f), grad(npix * 3, 0.f);
    drt_render_params rp = detail::render_params(tracer.absorb(), tracer.min_bounces(), spp, opt, detail::f64_flag(opt));
    rp.bounces_per_launch = 0;      // NOT the caller's: the gradient image keeps the route the library picks (>= 1 would move it to the queues)
    drt_hip_stats st{};
    detail::Session s = detail::Session::on_first_device(opt, flat);
    s.ctx.check(drt_hip_render_gradient_image(s.ctx.get(), &cd, &rp, index, nullptr, rgb.data(), grad.data(), &st),
                "drt_hip_render_gradient_image");
    detail::from_buffer(rgb.data(), npix, img);
    detail::from_buffer(grad.data(), npix, gimg);
    return detail::to_stats(st);
}

// ---- forward mode ----------------------------------------------------------------------------------------------
namespace detail {
// one drt_hip_render_tangent of a flattened scene along `v` (n_params x 3): both images in double (opt.f64: the device's own
// sums, drt_hip_render_tangent_double; else its float images).  Single device.
template <typename T>
inline Stats tangent_call(const char* who, const FlatScene<T>& flat, const drt_camera_desc& cd, double absorb, std::size_t min_bounces,
                          std::size_t spp, const std::vector<double>& v, std::vector<double>& img, std::vector<double>& timg,
                          const Options& opt)
{
    forward_only(who, opt, "forward mode");
    const std::size_t n = (std::size_t)cd.width * (std::size_t)cd.height * 3;
    const drt_render_params rp = render_params(absorb, min_bounces, spp, opt, f64_flag(opt));
    drt_hip_stats st{};
    Session s = Session::on_first_device(opt, flat);
    if (opt.f64) {
        img.assign(n, 0.0);
        timg.assign(n, 0.0);
        s.ctx.check(drt_hip_render_tangent_double(s.ctx.get(), &cd, &rp, v.data(), img.data(), timg.data(), &st), "drt_hip_render_tangent_double");
    } else {
        std::vector<float> rgb(n, 0.f), trgb(n, 0.f);
        s.ctx.check(drt_hip_render_tangent(s.ctx.get(), &cd, &rp, v.data(), rgb.data(), trgb.data(), &st), "drt_hip_render_tangent");
        img.assign(rgb.begin(), rgb.end());
        timg.assign(trgb.begin(), trgb.end());
    }
    return to_stats(st);
}
} // namespace detail

// J v: tangent_img[pixel] = mean over the pixel's samples of d radiance / d eps at params + eps * direction, `tangents` pairing
// parameter handles with their directions (handles not listed: direction 0; a listed handle the scene does not use throws, as
// render_gradient_image does; one listed twice adds up).  img may be nullptr.
template <typename T>
inline Stats render_tangent(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                            const std::vector<std::pair<Vector<T, 3, true>, Vector<T, 3>>>& tangents, Vector<T, 3>* img,
                            Vector<T, 3>* tangent_img, const Options& opt = Options())
{
    FlatScene<T> flat = flatten(scene);
    const std::vector<double> v = detail::rows_of("drt::hip::render_tangent", flat, std::vector<std::decay_t<decltype(tangents)>>{tangents}, nullptr, true,
                                                  [](const auto& t) { return std::make_pair(&t.first, &t.second); });
    std::vector<double> rgb, trgb;
    const Stats st = detail::tangent_call("drt::hip::render_tangent", flat, describe(cam), tracer.absorb(), tracer.min_bounces(), spp, v, rgb, trgb, opt);
    const std::size_t npix = cam.width() * cam.height();
    detail::from_buffer(rgb.data(), npix, img);
    detail::from_buffer(trgb.data(), npix, tangent_img);
    return st;
}

// ---- the Gauss-Newton normal equations of a frame (drt_hip_render_normal_equations) --------------------------------
// Per colour channel ch (channels do not mix): A[ch] = J^T J (P x P, row-major), b[ch] = J^T r, loss[ch] = r . r over the frame's pixels,
// with J the per-pixel derivative of the radiance with respect to that channel of every parameter of the scene, in the order of
// `handles` (FlatScene's: the order the scene's shapes name them).
template <typename T>
struct NormalEquations {
    std::size_t n_params = 0;
    std::vector<double> A, b, loss;             // 3 x P x P, 3 x P, 3
    std::vector<uint8_t> requires_grad;         // per parameter: rows that take part in solve()
    std::vector<Vector<T, 3, true>> handles;    // the parameters, sharing the scene's nodes
    Stats stats;

    // The Levenberg-Marquardt step: per channel, (A + lambda diag A) step = -b over the rows that require gradients, by a Cholesky
    // factorisation.  -> the step per (handle, channel), step[p * 3 + ch]; 0 for rows that require none.  Throws where the damped
    // matrix of a channel is not positive definite (a parameter no pixel depends on: give it lambda > 0 and a nonzero diagonal, or
    // requires_grad = false).
    std::vector<double> solve(double lambda) const
    {
        const std::size_t P = n_params;
        std::vector<double> step(P * 3, 0.0);
        std::vector<std::size_t> rows;
        for (std::size_t p = 0; p < P; ++p)
            if (p >= requires_grad.size() || requires_grad[p])
                rows.push_back(p);
        for (std::size_t ch = 0; ch < 3; ++ch) {
            const std::vector<double> x = detail::damped_cholesky(A.data() + ch * P * P, b.data() + ch * P, P, rows, lambda,
                                                                  "drt::hip::NormalEquations::solve: the damped matrix of a channel is not positive definite");
            for (std::size_t i = 0; i < rows.size(); ++i)
                step[rows[i] * 3 + ch] = x[i];
        }
        return step;
    }
};

// What the residual of normal_equations() is taken from: a target image (r = this render's own pixel means - target: one render per
// step, J and r share their samples) or the caller's residual (e.g. from an independently seeded forward render)
template <typename T>
struct TargetOrResidual {
    const Vector<T, 3>* image = nullptr;   // width x height
    bool is_residual = false;
    static TargetOrResidual target(const Vector<T, 3>* img) { TargetOrResidual t; t.image = img; return t; }
    static TargetOrResidual residual(const Vector<T, 3>* img) { TargetOrResidual t; t.image = img; t.is_residual = true; return t; }
};

// One render -> A, b, loss.  Single device; throws (std::runtime_error, with the library's message: "normal equations") where the
// device refuses: more than 8 parameters, a mesh, bounces_per_launch >= 1, the reverse-mode options, several devices.
template <typename T>
inline NormalEquations<T> normal_equations(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                                           const Options& opt, const TargetOrResidual<T>& target_or_residual, Vector<T, 3>* img = nullptr)
{
    if (opt.backward || opt.unbiased || opt.sample_loss_l2)
        throw std::runtime_error("drt::hip::normal_equations: the normal equations take no reverse-mode option (backward, unbiased, sample_loss_l2)");
    if (opt.devices.size() > 1)
        throw std::runtime_error("drt::hip::normal_equations: the normal equations come from one device (render shards on plain contexts and add them)");
    if (!target_or_residual.image)
        throw std::runtime_error("drt::hip::normal_equations: the normal equations need a target or a residual image");
    FlatScene<T> flat = flatten(scene);
    const drt_camera_desc cd = describe(cam);
    const std::size_t npix = cam.width() * cam.height(), P = flat.handles.size();
    const std::vector<float> in = detail::to_floats(target_or_residual.image, npix);
    std::vector<float> rgb(npix * 3, 0.f);
    NormalEquations<T> ne;
    ne.n_params = P;
    ne.A.assign(3 * P * P, 0.0);
    ne.b.assign(3 * P, 0.0);
    ne.loss.assign(3, 0.0);
    ne.requires_grad = flat.requires_grad;
    ne.handles = flat.handles;
    const drt_render_params rp = detail::render_params(tracer.absorb(), tracer.min_bounces(), spp, opt, detail::f64_flag(opt));
    drt_hip_stats st{};
    std::vector<double> dummy(1);
    detail::Session s = detail::Session::on_first_device(opt, flat);
    s.ctx.check(drt_hip_render_normal_equations(s.ctx.get(), &cd, &rp, target_or_residual.is_residual ? nullptr : in.data(),
                                                target_or_residual.is_residual ? in.data() : nullptr, rgb.data(), P ? ne.A.data() : dummy.data(),
                                                P ? ne.b.data() : dummy.data(), ne.loss.data(), nullptr, &st),
                "drt_hip_render_normal_equations");
    detail::from_buffer(rgb.data(), npix, img);
    ne.stats = detail::to_stats(st);
    return ne;
}

// ---- K directions in one render (drt_hip_render_tangents / drt_hip_render_normal_equations_along) -------------------
// A direction of parameter space as render_tangent takes it: (handle, direction) pairs; handles not listed have direction 0
template <typename T>
using Direction = std::vector<std::pair<Vector<T, 3, true>, Vector<T, 3>>>;

namespace detail {
// K directions as the ABI takes them, K x n_params x 3
template <typename T>
inline std::vector<double> directions_of(const char* who, const FlatScene<T>& flat, const std::vector<Direction<T>>& directions)
{
    return rows_of(who, flat, directions, nullptr, true, [](const auto& t) { return std::make_pair(&t.first, &t.second); });
}
// the one call behind render_tangents and normal_equations_along: A, b, loss where `in` is given, the K images where `timg` is
template <typename T>
inline Stats tangents_call(const char* who, const FlatScene<T>& flat, const drt_camera_desc& cd, double absorb, std::size_t min_bounces,
                           std::size_t spp, std::size_t K, const std::vector<double>& v, const float* in, bool in_is_residual,
                           std::vector<float>& rgb, std::vector<float>* timg, double* A, double* b, double* loss, const Options& opt)
{
    forward_only(who, opt, "forward mode");
    one_device(who, opt);
    const std::size_t n = (std::size_t)cd.width * (std::size_t)cd.height * 3;
    rgb.assign(n, 0.f);
    if (timg)
        timg->assign((K ? K : 1) * n, 0.f);
    const drt_render_params rp = render_params(absorb, min_bounces, spp, opt, f64_flag(opt));
    drt_hip_stats st{};
    Session s = Session::on_first_device(opt, flat);
    if (A)
        s.ctx.check(drt_hip_render_normal_equations_along(s.ctx.get(), &cd, &rp, (int32_t)K, v.data(), in_is_residual ? nullptr : in,
                                                          in_is_residual ? in : nullptr, rgb.data(), A, b, loss, timg ? timg->data() : nullptr, &st),
                    "drt_hip_render_normal_equations_along");
    else
        s.ctx.check(drt_hip_render_tangents(s.ctx.get(), &cd, &rp, (int32_t)K, v.data(), rgb.data(), timg ? timg->data() : nullptr, &st),
                    "drt_hip_render_tangents");
    return to_stats(st);
}
} // namespace detail

// J v_k for up to DRT_HIP_MAX_DIRS directions in one render: tangent_imgs[k * width * height + pixel] is what render_tangent gives for
// directions[k] (the device's float images; with opt.f64 its double sums, rounded).  img may be nullptr.
template <typename T>
inline Stats render_tangents(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                             const std::vector<Direction<T>>& directions, Vector<T, 3>* img, Vector<T, 3>* tangent_imgs,
                             const Options& opt = Options())
{
    FlatScene<T> flat = flatten(scene);
    const std::vector<double> v = detail::directions_of("drt::hip::render_tangents", flat, directions);
    std::vector<float> rgb, trgb;
    const Stats st = detail::tangents_call("drt::hip::render_tangents", flat, describe(cam), tracer.absorb(), tracer.min_bounces(), spp,
                                           directions.size(), v, nullptr, false, rgb, &trgb, nullptr, nullptr, nullptr, opt);
    const std::size_t npix = cam.width() * cam.height();
    detail::from_buffer(rgb.data(), npix, img);
    detail::from_buffer(trgb.data(), npix * directions.size(), tangent_imgs);
    return st;
}

// The normal equations in the span of K directions: per channel A[ch] = V^T J^T J V (K x K, row-major), b[ch] = V^T J^T r,
// loss[ch] = r . r -- for a scene of any number of parameters the path kernels stage.  solve() gives the Levenberg-Marquardt step in
// the directions' coordinates, step[k * 3 + ch]: the parameters move by sum_k step[k * 3 + ch] directions[k].
// A direction that leaves a channel alone -- d theta / d tint_red in green -- has a zero diagonal there: solve() keeps such a row out of
// that channel's system and returns step 0 for it.
template <typename T>
struct NormalEquationsAlong {
    std::size_t n_dirs = 0;
    std::vector<double> A, b, loss;             // 3 x K x K, 3 x K, 3
    Stats stats;
    std::vector<double> solve(double lambda) const
    {
        // (NormalEquations::solve's step, with the rows chosen per channel: those whose diagonal is positive)
        const std::size_t K = n_dirs;
        std::vector<double> step(K * 3, 0.0);
        for (std::size_t ch = 0; ch < 3; ++ch) {
            const double* Ac = A.data() + ch * K * K;
            std::vector<std::size_t> rows;
            for (std::size_t k = 0; k < K; ++k)
                if (Ac[k * K + k] > 0.0)
                    rows.push_back(k);
            const std::vector<double> x = detail::damped_cholesky(Ac, b.data() + ch * K, K, rows, lambda,
                                                                  "drt::hip::NormalEquationsAlong::solve: the damped matrix of a channel is not positive "
                                                                  "definite (linearly dependent directions: give it lambda > 0)");
            for (std::size_t i = 0; i < rows.size(); ++i)
                step[rows[i] * 3 + ch] = x[i];
        }
        return step;
    }
};

template <typename T>
inline NormalEquationsAlong<T> normal_equations_along(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                                                      const std::vector<Direction<T>>& directions, const Options& opt,
                                                      const TargetOrResidual<T>& target_or_residual, Vector<T, 3>* img = nullptr,
                                                      Vector<T, 3>* tangent_imgs = nullptr)
{
    if (!target_or_residual.image)
        throw std::runtime_error("drt::hip::normal_equations_along: the normal equations need a target or a residual image");
    FlatScene<T> flat = flatten(scene);
    const std::vector<double> v = detail::directions_of("drt::hip::normal_equations_along", flat, directions);
    const std::size_t npix = cam.width() * cam.height(), K = directions.size();
    const std::vector<float> in = detail::to_floats(target_or_residual.image, npix);
    NormalEquationsAlong<T> ne;
    ne.n_dirs = K;
    ne.A.assign(3 * (K ? K * K : 1), 0.0);
    ne.b.assign(3 * (K ? K : 1), 0.0);
    ne.loss.assign(3, 0.0);
    std::vector<float> rgb, trgb;
    ne.stats = detail::tangents_call("drt::hip::normal_equations_along", flat, describe(cam), tracer.absorb(), tracer.min_bounces(), spp, K, v,
                                     in.data(), target_or_residual.is_residual, rgb, tangent_imgs ? &trgb : nullptr, ne.A.data(), ne.b.data(),
                                     ne.loss.data(), opt);
    detail::from_buffer(rgb.data(), npix, img);
    if (tangent_imgs)
        detail::from_buffer(trgb.data(), npix * K, tangent_imgs);
    return ne;
}

// ... with b and the loss unbiased from this ONE render (drt_hip_render_normal_equations_cross): the products of each pixel's means less
// the sample covariance of its samples over spp -- the mean over ordered pairs of DIFFERENT samples, whose expectation is the product of
// the expectations.  A is NormalEquationsAlong's (its Cov / spp excess is positive semi-definite: damping).  bias[ch * (K + 1) + k] is what
// was subtracted from b[ch * K + k], bias[ch * (K + 1) + K] what was subtracted from loss[ch]: the render's own noise floor.  variance
// (width x height x 3, where asked for) is the variance of each pixel's mean.
template <typename T>
struct NormalEquationsCross : NormalEquationsAlong<T> {
    std::vector<double> bias;                   // 3 x (K + 1)
    std::vector<float> variance;                // width x height x 3, or empty
};

template <typename T>
inline NormalEquationsCross<T> normal_equations_cross(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                                                      const std::vector<Direction<T>>& directions, const Options& opt, const Vector<T, 3>* target,
                                                      Vector<T, 3>* img = nullptr, Vector<T, 3>* tangent_imgs = nullptr, bool want_variance = false)
{
    const char* who = "drt::hip::normal_equations_cross";
    if (!target)
        throw std::runtime_error("drt::hip::normal_equations_cross: the cross-sample normal equations need a target image");
    if (spp < 2)
        throw std::runtime_error("drt::hip::normal_equations_cross: spp < 2 (the estimator needs a pair of samples per pixel)");
    detail::forward_only(who, opt, "forward mode");
    detail::one_device(who, opt);
    FlatScene<T> flat = flatten(scene);
    const std::vector<double> v = detail::directions_of(who, flat, directions);
    const drt_camera_desc cd = describe(cam);
    const std::size_t npix = cam.width() * cam.height(), K = directions.size();
    const std::vector<float> in = detail::to_floats(target, npix);
    NormalEquationsCross<T> ne;
    ne.n_dirs = K;
    ne.A.assign(3 * (K ? K * K : 1), 0.0);
    ne.b.assign(3 * (K ? K : 1), 0.0);
    ne.loss.assign(3, 0.0);
    ne.bias.assign(3 * (K + 1), 0.0);
    if (want_variance)
        ne.variance.assign(npix * 3, 0.f);
    std::vector<float> rgb(npix * 3, 0.f), trgb;
    if (tangent_imgs)
        trgb.assign((K ? K : 1) * npix * 3, 0.f);
    const drt_render_params rp = detail::render_params(tracer.absorb(), tracer.min_bounces(), spp, opt, detail::f64_flag(opt));
    drt_hip_stats st{};
    {
        detail::Session s = detail::Session::on_first_device(opt, flat);
        s.ctx.check(drt_hip_render_normal_equations_cross(s.ctx.get(), &cd, &rp, (int32_t)K, v.data(), in.data(), rgb.data(), ne.A.data(), ne.b.data(),
                                                          ne.loss.data(), ne.bias.data(), tangent_imgs ? trgb.data() : nullptr,
                                                          want_variance ? ne.variance.data() : nullptr, &st),
                    "drt_hip_render_normal_equations_cross");
    }
    ne.stats = detail::to_stats(st);
    detail::from_buffer(rgb.data(), npix, img);
    if (tangent_imgs)
        detail::from_buffer(trgb.data(), npix * K, tangent_imgs);
    return ne;
}

// ---- one frame under several parameter sets in one trace (drt_hip_render_param_sets) ------------------------------------
// A parameter set as render_tangent takes a direction: (handle, value) pairs over the scene's current values; handles not listed keep
// the value they have in the scene
template <typename T>
using ParamSet = std::vector<std::pair<Vector<T, 3, true>, Vector<T, 3>>>;

namespace detail {
// the one call behind render_param_sets and render_param_sets_along: the target as floats, the image buffers, the caller's entry point
// `abi(context, camera, render parameters, target, images, derivative images, statistics)` on the first device, the images back
template <typename T, typename Abi>
inline Stats sets_call(const char* abi_name, const FlatScene<T>& flat, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                       std::size_t K, const Vector<T, 3>* target, Vector<T, 3>* imgs, Vector<T, 3>* tangent_imgs, const Options& opt, Abi abi)
{
    const drt_camera_desc cd = describe(cam);
    const std::size_t npix = cam.width() * cam.height();
    std::vector<float> tgt, out, tout;
    if (target)
        tgt = to_floats(target, npix);
    if (imgs)
        out.assign((K ? K : 1) * npix * 3, 0.f);
    if (tangent_imgs)
        tout.assign((K ? K : 1) * npix * 3, 0.f);
    const drt_render_params rp = render_params(tracer.absorb(), tracer.min_bounces(), spp, opt, f64_flag(opt));
    drt_hip_stats st{};
    {
        Session s = Session::on_first_device(opt, flat);
        s.ctx.check(abi(s.ctx.get(), &cd, &rp, target ? tgt.data() : nullptr, imgs ? out.data() : nullptr, tangent_imgs ? tout.data() : nullptr, &st),
                    abi_name);
    }
    if (imgs)
        from_buffer(out.data(), npix * K, imgs);
    if (tangent_imgs)
        from_buffer(tout.data(), npix * K, tangent_imgs);
    return to_stats(st);
}
} // namespace detail

// What a frame looks like, and what its loss is, under each of up to DRT_HIP_MAX_PARAM_SETS parameter sets: imgs[k * width * height +
// pixel] is what render() gives with sets[k] installed (nullptr: no images), losses[k * 3 + ch] the sum over the pixels of
// (mean_k - target)^2 where `target` (width x height) is given, empty otherwise.  The scene's own values are not changed.
template <typename T>
inline Stats render_param_sets(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                               const std::vector<ParamSet<T>>& sets, const Vector<T, 3>* target, Vector<T, 3>* imgs,
                               std::vector<double>* losses, const Options& opt = Options())
{
    const char* who = "drt::hip::render_param_sets";
    detail::forward_only(who, opt, "a forward render");
    detail::one_device(who, opt);
    if (!imgs && !(losses && target))
        throw std::runtime_error(std::string(who) + ": no output requested (images, or losses with a target)");
    if (losses && !target)
        throw std::runtime_error(std::string(who) + ": losses need a target");
    FlatScene<T> flat = flatten(scene);
    const std::size_t K = sets.size();
    const std::vector<double> values =
        detail::rows_of(who, flat, sets, flat.params.data(), false, [](const auto& t) { return std::make_pair(&t.first, &t.second); });
    if (losses)
        losses->assign(K * 3, 0.0);
    return detail::sets_call("drt_hip_render_param_sets", flat, cam, tracer, spp, K, target, imgs, (Vector<T, 3>*)nullptr, opt,
                             [&](drt_hip_ctx* ctx, const drt_camera_desc* cd, const drt_render_params* rp, const float* tgt, float* out, float*,
                                 drt_hip_stats* st) {
                                 return drt_hip_render_param_sets(ctx, cd, rp, (int32_t)K, values.data(), tgt, out,
                                                                  (losses && K) ? losses->data() : nullptr, nullptr, st);
                             });
}

// ---- ... each set's loss unbiased (drt_hip_render_param_sets_cross) -------------------------------------------------------------
// The loss of the frame under each of up to DRT_HIP_MAX_SETS_CROSS parameter sets, from one trace, without the share the samples' noise
// adds to a squared residual: with m_k the pixel's mean over its n = spp samples, r_k = m_k - target and var^ their sample variance, per
// set and channel (index k * 3 + ch)
//     losses = sum (r_k^2 - var^(L_k) / n)      biases = sum var^(L_k) / n      (losses + biases: render_param_sets' losses)
// imgs (nullptr: none): render_param_sets' images; variance_imgs (nullptr: none): [k * width * height + pixel] var^(L_k) / n.  spp < 2 and
// a missing target throw before a device is asked for.  The scene's own values are not changed.
template <typename T>
struct SetsCross {
    std::vector<double> losses, biases;
    Stats stats;
};

template <typename T>
inline SetsCross<T> render_param_sets_cross(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                                            const std::vector<ParamSet<T>>& sets, const Vector<T, 3>* target, Vector<T, 3>* imgs = nullptr,
                                            Vector<T, 3>* variance_imgs = nullptr, const Options& opt = Options())
{
    const char* who = "drt::hip::render_param_sets_cross";
    detail::forward_only(who, opt, "a forward render");
    detail::one_device(who, opt);
    if (spp < 2)
        throw std::runtime_error(std::string(who) + ": spp < 2 (a product of two different samples of a pixel needs two)");
    if (!target)
        throw std::runtime_error(std::string(who) + ": the unbiased losses need a target");
    FlatScene<T> flat = flatten(scene);
    const std::size_t K = sets.size();
    const std::vector<double> values =
        detail::rows_of(who, flat, sets, flat.params.data(), false, [](const auto& t) { return std::make_pair(&t.first, &t.second); });
    SetsCross<T> r;
    r.losses.assign(K * 3, 0.0);
    r.biases.assign(K * 3, 0.0);
    r.stats = detail::sets_call("drt_hip_render_param_sets_cross", flat, cam, tracer, spp, K, target, imgs, variance_imgs, opt,
                                [&](drt_hip_ctx* ctx, const drt_camera_desc* cd, const drt_render_params* rp, const float* tgt, float* out, float* vout,
                                    drt_hip_stats* st) {
                                    return drt_hip_render_param_sets_cross(ctx, cd, rp, (int32_t)K, values.data(), tgt, out, K ? r.losses.data() : nullptr,
                                                                           K ? r.biases.data() : nullptr, vout, st);
                                });
    return r;
}

// ---- ... each set with a direction of its own (drt_hip_render_param_sets_along) ----------------------------------------------
// A parameter set with its direction: (handle, value, direction) triples over the scene's current values; handles not listed keep the
// value they have in the scene and get direction 0
template <typename T>
struct ParamAlong {
    Vector<T, 3, true> handle;
    Vector<T, 3> value, direction;
};
template <typename T>
using ParamSetAlong = std::vector<ParamAlong<T>>;

// Value, slope and Gauss-Newton curvature of the loss under each of up to DRT_HIP_MAX_SETS_ALONG parameter sets, each along its own
// direction, from one trace: with r_k = mean_k - target and t_k = J(P_k) d_k, per set and channel (index k * 3 + ch)
//     losses = sum r_k^2      slopes = sum 2 r_k t_k      curvatures = sum t_k^2
// losses and slopes are empty without a target.  imgs / tangent_imgs (nullptr: none): [k * width * height + pixel] what render() and
// render_tangent() give with sets[k] installed.  The scene's own values are not changed.
template <typename T>
struct SetsAlong {
    std::vector<double> losses, slopes, curvatures;
    Stats stats;
};

template <typename T>
inline SetsAlong<T> render_param_sets_along(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                                            const std::vector<ParamSetAlong<T>>& sets, const Vector<T, 3>* target, Vector<T, 3>* imgs = nullptr,
                                            Vector<T, 3>* tangent_imgs = nullptr, const Options& opt = Options())
{
    const char* who = "drt::hip::render_param_sets_along";
    detail::forward_only(who, opt, "a forward render");
    detail::one_device(who, opt);
    FlatScene<T> flat = flatten(scene);
    const std::size_t K = sets.size();
    const std::vector<double> values =
        detail::rows_of(who, flat, sets, flat.params.data(), false, [](const auto& t) { return std::make_pair(&t.handle, &t.value); });
    const std::vector<double> dirs = detail::rows_of(who, flat, sets, nullptr, false, [](const auto& t) { return std::make_pair(&t.handle, &t.direction); });
    SetsAlong<T> r;
    if (target) {
        r.losses.assign(K * 3, 0.0);
        r.slopes.assign(K * 3, 0.0);
    }
    r.curvatures.assign(K * 3, 0.0);
    r.stats = detail::sets_call("drt_hip_render_param_sets_along", flat, cam, tracer, spp, K, target, imgs, tangent_imgs, opt,
                                [&](drt_hip_ctx* ctx, const drt_camera_desc* cd, const drt_render_params* rp, const float* tgt, float* out, float* tout,
                                    drt_hip_stats* st) {
                                    return drt_hip_render_param_sets_along(ctx, cd, rp, (int32_t)K, values.data(), dirs.data(), tgt, out, tout,
                                                                           (target && K) ? r.losses.data() : nullptr,
                                                                           (target && K) ? r.slopes.data() : nullptr,
                                                                           K ? r.curvatures.data() : nullptr, st);
                                });
    return r;
}

// ---- ... each set's summed gradient (drt_hip_render_param_sets_grad) -----------------------------------------------------------
// The gradient of the frame under each of up to DRT_HIP_MAX_SETS_GRAD parameter sets, from one trace: grads[k] lists every parameter of
// the scene with d <adjoint_k, radiance sum> / d parameter at sets[k] -- what render() with Options::backward leaves in the handles' grad()
// with sets[k] installed and adjoints + k * width * height as the adjoint image, as the sum over the samples; zero for a handle that
// requires no gradient.  `adjoints` (sets.size() x width x height; nullptr: every seed (1, 1, 1)).  Handles a set does not list keep the
// scene's value; a listed handle the scene does not use throws.  The scene's own values and gradients are not changed.
template <typename T>
struct SetsGrad {
    std::vector<ParamSet<T>> grads;     // per set: (handle, gradient) for every parameter of the scene, in the scene's order
    Stats stats;
};

template <typename T>
inline SetsGrad<T> render_param_sets_grad(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                                          const std::vector<ParamSet<T>>& sets, const Vector<T, 3>* adjoints = nullptr, const Options& opt = Options())
{
    const char* who = "drt::hip::render_param_sets_grad";
    if (opt.unbiased || opt.sample_loss_l2)
        throw std::runtime_error(std::string(who) + ": the biased operator's summed gradients (backward is implied; no unbiased, no sample_loss_l2)");
    detail::one_device(who, opt);
    FlatScene<T> flat = flatten(scene);
    const std::size_t K = sets.size(), n = flat.handles.size(), npix = cam.width() * cam.height();
    const std::vector<double> values =
        detail::rows_of(who, flat, sets, flat.params.data(), false, [](const auto& t) { return std::make_pair(&t.first, &t.second); });
    std::vector<float> seeds;
    if (adjoints)
        seeds = detail::to_floats(adjoints, npix * K);
    std::vector<double> sums((K * n ? K * n : 1) * 3, 0.0);
    Options forward = opt;
    forward.backward = false;           // (implied by the call: the flag itself is the entry point's to add or not)
    SetsGrad<T> r;
    r.stats = detail::sets_call("drt_hip_render_param_sets_grad", flat, cam, tracer, spp, K, (const Vector<T, 3>*)nullptr, (Vector<T, 3>*)nullptr,
                                (Vector<T, 3>*)nullptr, forward,
                                [&](drt_hip_ctx* ctx, const drt_camera_desc* cd, const drt_render_params* rp, const float*, float*, float*,
                                    drt_hip_stats* st) {
                                    return drt_hip_render_param_sets_grad(ctx, cd, rp, (int32_t)K, values.data(), adjoints ? seeds.data() : nullptr,
                                                                          sums.data(), st);
                                });
    r.grads.resize(K);
    for (std::size_t k = 0; k < K; ++k)
        for (std::size_t p = 0; p < n; ++p)
            r.grads[k].emplace_back(flat.handles[p], Vector<T, 3>{T(sums[(k * n + p) * 3]), T(sums[(k * n + p) * 3 + 1]), T(sums[(k * n + p) * 3 + 2])});
    return r;
}

// ---- one scene from several cameras in one trace (drt_hip_render_views) ----------------------------------------------------------------
// render() for up to DRT_HIP_MAX_VIEWS cameras of one size at once: images[v * width * height + pixel] is what render() with cameras[v]
// leaves in its img, bit for bit; with Options::backward the SUM over the views of what those calls add to the handles' grad() is added to
// them (the views' gradients added in view order), adjoints + v * width * height view v's adjoint image (nullptr: all ones).  `seeds`
// (one per view; empty: Options::seed for every view).  One device; the biased operator.  Throws what render() throws for a scene it
// cannot flatten.
template <typename T>
inline Stats render_views(const Scene<T>& scene, const std::vector<Camera<T>>& cameras, const Pathtracer<T>& tracer, std::size_t spp,
                          Vector<T, 3>* images, const Options& opt = Options(), const Vector<T, 3>* adjoints = nullptr,
                          const std::vector<uint32_t>& seeds = std::vector<uint32_t>())
{
    const char* who = "drt::hip::render_views";
    if (opt.unbiased || opt.sample_loss_l2)
        throw std::runtime_error(std::string(who) + ": the biased operator (no unbiased, no sample_loss_l2)");
    detail::one_device(who, opt);
    if (cameras.empty() || cameras.size() > (std::size_t)DRT_HIP_MAX_VIEWS)
        throw std::runtime_error(std::string(who) + ": 1 ... DRT_HIP_MAX_VIEWS = 64 cameras");
    if (!seeds.empty() && seeds.size() != cameras.size())
        throw std::runtime_error(std::string(who) + ": a seed per camera, or none");
    FlatScene<T> flat = flatten(scene);
    const std::size_t V = cameras.size(), npix = cameras[0].width() * cameras[0].height();
    std::vector<drt_camera_desc> cds;
    for (const Camera<T>& cam : cameras) {
        if (cam.width() != cameras[0].width() || cam.height() != cameras[0].height())
            throw std::runtime_error(std::string(who) + ": the cameras differ in width or height (all views share one size)");
        cds.push_back(describe(cam));
    }
    const std::vector<float> adj = adjoints && opt.backward ? detail::to_floats(adjoints, npix * V) : std::vector<float>();
    const drt_render_params rp = detail::render_params(tracer.absorb(), tracer.min_bounces(), spp, opt, detail::reverse_flags(opt));
    std::vector<double> grads((flat.requires_grad.size() ? flat.requires_grad.size() : 1) * 3, 0.0);
    std::vector<float> frames(images ? npix * 3 * V : 0, 0.f);
    if (!images && !opt.backward)
        throw std::runtime_error(std::string(who) + ": nothing to compute (no images, no backward)");
    drt_hip_stats st{};
    {
        detail::Session s = detail::Session::on_first_device(opt, flat);
        s.ctx.check(drt_hip_render_views(s.ctx.get(), cds.data(), (int32_t)V, &rp, seeds.empty() ? nullptr : seeds.data(),
                                         adj.empty() ? nullptr : adj.data(), images ? frames.data() : nullptr,
                                         opt.backward ? grads.data() : nullptr, nullptr, &st),
                    "drt_hip_render_views");
    }
    if (images)
        detail::from_buffer(frames.data(), npix * V, images);
    if (opt.backward)
        detail::accumulate_grads(flat.handles, flat.requires_grad, grads.data());
    return detail::to_stats(st);
}

// ---- a caller's batch of pixels from several cameras in one trace (drt_hip_render_pixels) ---------------------------------------------
// render_views() for pixel lists: pixels[v] holds camera v's pixels as y * width + x, in any order, repeats allowed, possibly none; out gets
// one value per entry in list order, the views' lists one behind the other -- that pixel of what render() with cameras[v] leaves in its
// img, bit for bit; with Options::backward the SUM over all entries of what their samples add to the handles' grad() is added to them,
// adjoints[e] entry e's adjoint (nullptr: all ones).  `seeds` (one per view; empty: Options::seed for every view).  One device; the biased
// operator.  Throws where render_views() throws, and on an empty batch and on a pixel outside the frame.
template <typename T>
inline Stats render_pixels(const Scene<T>& scene, const std::vector<Camera<T>>& cameras, const std::vector<std::vector<uint32_t>>& pixels,
                           const Pathtracer<T>& tracer, std::size_t spp, Vector<T, 3>* out, const Options& opt = Options(),
                           const Vector<T, 3>* adjoints = nullptr, const std::vector<uint32_t>& seeds = std::vector<uint32_t>())
{
    const char* who = "drt::hip::render_pixels";
    if (opt.unbiased || opt.sample_loss_l2)
        throw std::runtime_error(std::string(who) + ": the biased operator (no unbiased, no sample_loss_l2)");
    detail::one_device(who, opt);
    if (cameras.empty() || cameras.size() > (std::size_t)DRT_HIP_MAX_VIEWS)
        throw std::runtime_error(std::string(who) + ": 1 ... DRT_HIP_MAX_VIEWS = 64 cameras");
    if (pixels.size() != cameras.size())
        throw std::runtime_error(std::string(who) + ": a pixel list per camera");
    if (!seeds.empty() && seeds.size() != cameras.size())
        throw std::runtime_error(std::string(who) + ": a seed per camera, or none");
    const std::size_t V = cameras.size(), npix = cameras[0].width() * cameras[0].height();
    std::vector<int32_t> counts;
    std::vector<uint32_t> list;
    for (const std::vector<uint32_t>& l : pixels) {
        counts.push_back((int32_t)l.size());
        for (uint32_t p : l) {
            if ((std::size_t)p >= npix)
                throw std::runtime_error(std::string(who) + ": a pixel outside the frame (>= width * height)");
            list.push_back(p);
        }
    }
    if (list.empty())
        throw std::runtime_error(std::string(who) + ": an empty batch (no entries in any view)");
    FlatScene<T> flat = flatten(scene);
    std::vector<drt_camera_desc> cds;
    for (const Camera<T>& cam : cameras) {
        if (cam.width() != cameras[0].width() || cam.height() != cameras[0].height())
            throw std::runtime_error(std::string(who) + ": the cameras differ in width or height (all views share one size)");
        cds.push_back(describe(cam));
    }
    const std::size_t E = list.size();
    const std::vector<float> adj = adjoints && opt.backward ? detail::to_floats(adjoints, E) : std::vector<float>();
    const drt_render_params rp = detail::render_params(tracer.absorb(), tracer.min_bounces(), spp, opt, detail::reverse_flags(opt));
    std::vector<double> grads((flat.requires_grad.size() ? flat.requires_grad.size() : 1) * 3, 0.0);
    std::vector<float> rgb(out ? E * 3 : 0, 0.f);
    if (!out && !opt.backward)
        throw std::runtime_error(std::string(who) + ": nothing to compute (no out, no backward)");
    drt_hip_stats st{};
    {
        detail::Session s = detail::Session::on_first_device(opt, flat);
        s.ctx.check(drt_hip_render_pixels(s.ctx.get(), cds.data(), (int32_t)V, &rp, seeds.empty() ? nullptr : seeds.data(), counts.data(), list.data(),
                                          adj.empty() ? nullptr : adj.data(), out ? rgb.data() : nullptr,
                                          opt.backward ? grads.data() : nullptr, nullptr, &st),
                    "drt_hip_render_pixels");
    }
    if (out)
        detail::from_buffer(rgb.data(), E, out);
    if (opt.backward)
        detail::accumulate_grads(flat.handles, flat.requires_grad, grads.data());
    return detail::to_stats(st);
}

// ---- the per-sample loss from the caller's own source (drt_hip_set_sample_loss / drt_hip_render_sample_loss) ------------------------
// The reference's loop -- radiance = tracer.trace(...); loss = loss_func(radiance); loss.backward() (README.md:93-98) -- with loss_func the
// caller's: `src` is the body of
//     template <typename R> void sample_loss(const R* q, V3<R> L, V3<R> t, R& value, V3<R>& grad)
// (L one camera sample's radiance, t its pixel of `target`, value = loss_func(L), grad = d value / d L; helpers: csrc/drt_device.h),
// `values` its constants q[0 .. DRT_MAX_LOSS_VALUES) -- data: the same source with other values compiles nothing.  An empty `src`: the
// squared error.
struct SampleLoss {
    std::string name, src;
    std::vector<double> values;
};
struct SampleLossResult {
    Stats stats;
    double loss = 0.0;              // the sum of the samples' values over the frame
};
// One render under `loss`: backward is implied, the gradients are ADDED to the handles' .grad() as render does with Options::backward, `img`
// (may be nullptr) gets the plain mean image.  One device.  Options::backward is the call's own and is ignored; unbiased and sample_loss_l2
// make no sense here and throw, like more values than the ABI takes and a missing target, before a device is asked for.
template <typename T>
inline SampleLossResult render_sample_loss(const Scene<T>& scene, const Camera<T>& cam, const Pathtracer<T>& tracer, std::size_t spp,
                                           const Vector<T, 3>* target, Vector<T, 3>* img, const SampleLoss& loss, const Options& opt = Options())
{
    const char* who = "drt::hip::render_sample_loss";
    if (opt.unbiased || opt.sample_loss_l2)
        throw std::runtime_error(std::string(who) + ": the sample loss is the call's own -- no unbiased operator, no sample_loss_l2 beside it");
    detail::one_device(who, opt);
    if (!target)
        throw std::runtime_error(std::string(who) + ": a sample loss needs a target image");
    if (loss.values.size() > (std::size_t)DRT_MAX_LOSS_VALUES)
        throw std::runtime_error(std::string(who) + ": a sample loss takes at most DRT_MAX_LOSS_VALUES (4) values");
    FlatScene<T> flat = flatten(scene);
    const drt_camera_desc cd = describe(cam);
    const std::size_t npix = cam.width() * cam.height();
    const std::vector<float> tgt = detail::to_floats(target, npix);
    const drt_render_params rp = detail::render_params(tracer.absorb(), tracer.min_bounces(), spp, opt, detail::f64_flag(opt));
    drt_sample_loss_desc desc{};
    desc.name = loss.name.c_str();
    desc.loss_src = loss.src.c_str();
    for (std::size_t k = 0; k < loss.values.size(); ++k)
        desc.values[k] = loss.values[k];
    std::vector<double> grads(flat.requires_grad.size() * 3, 0.0);
    std::vector<float> frame(img ? npix * 3 : 0, 0.f);
    drt_hip_stats st{};
    SampleLossResult r;
    {
        detail::Session s = detail::Session::on_first_device(opt, flat);
        s.ctx.check(drt_hip_set_sample_loss(s.ctx.get(), loss.src.empty() ? nullptr : &desc), "drt_hip_set_sample_loss");
        const int rc = drt_hip_render_sample_loss(s.ctx.get(), &cd, &rp, tgt.data(), img ? frame.data() : nullptr, grads.data(), &r.loss, &st);
        (void)drt_hip_set_sample_loss(s.ctx.get(), nullptr);   // (a pooled context goes back with the default loss)
        s.ctx.check(rc, "drt_hip_render_sample_loss");
    }
    detail::from_buffer(frame.data(), npix, img);
    detail::accumulate_grads(flat.handles, flat.requires_grad, grads.data());
    r.stats = detail::to_stats(st);
    return r;
}

// A Scene<Dual<U>> for the device: the real parts as the scene, the dual parts of its PARAMETERS as the direction (n_params x 3).
// A nonzero dual part anywhere the device does not differentiate -- a plane's normal, a sphere's centre, a mesh's vertices --
// throws and names the field: a seed is never dropped silently.  (Offsets, radii, exponents and the tracer's absorb are plain
// doubles in this API: they cannot carry one.)
template <typename U>
inline FlatScene<Dual<U>> flatten_dual(const Scene<Dual<U>>& scene, std::vector<double>& tangent)
{
    std::size_t i = 0;
    for (Shape<Dual<U>>* shape : scene) {
        const ShapeRecord rec = shape->describe();
        for (int k = 0; k < 4; ++k)
            if (rec.dual[k] != 0)
                throw std::runtime_error("drt::hip: shape " + std::to_string(i) + " carries a dual part on its " +
                                         (rec.kind == ShapeKind::Plane ? "normal" : rec.kind == ShapeKind::Sphere ? "centre" : "record") +
                                         ": geometry is not differentiated on the device");
        if (auto* mesh = dynamic_cast<Mesh<Dual<U>>*>(shape))
            for (const auto& vtx : mesh->vertices())
                for (int c = 0; c < 3; ++c)
                    if (dual_part(vtx[c]) != U(0))
                        throw std::runtime_error("drt::hip: shape " + std::to_string(i) + " carries a dual part on a mesh vertex: geometry is not "
                                                 "differentiated on the device");
        ++i;
    }
    FlatScene<Dual<U>> flat = flatten(scene);
    tangent.assign(flat.handles.size() * 3, 0.0);
    for (std::size_t p = 0; p < flat.handles.size(); ++p)
        for (int c = 0; c < 3; ++c)
            tangent[p * 3 + c] = double(dual_part(flat.handles[p][c]));
    return flat;
}
template <typename U>
inline drt_camera_desc describe_dual(const Camera<Dual<U>>& cam)
{
    const char* names[4] = {"eye", "forward", "right", "up"};
    const Vector<Dual<U>, 3> vs[4] = {cam.eye(), cam.forward(), cam.right(), cam.up()};
    for (int k = 0; k < 4; ++k)
        for (int c = 0; c < 3; ++c)
            if (dual_part(vs[k][c]) != U(0))
                throw std::runtime_error(std::string("drt::hip: the camera carries a dual part on its ") + names[k] +
                                         ": the camera is not differentiated on the device");
    return describe(cam);
}

// T = Dual<U>: the reference's own validation run (its README: reverse mode "validated against ... forward mode"), on the device.
// img[pixel] = Dual(radiance, d radiance / d eps), eps the scene's dual unit.  Reverse-mode options and an adjoint image throw.
template <typename U>
inline Stats render(const Scene<Dual<U>>& scene, const Camera<Dual<U>>& cam, const Pathtracer<Dual<U>>& tracer, std::size_t spp,
                    Vector<Dual<U>, 3>* img, const Options& opt = Options(), const Vector<Dual<U>, 3>* adjoint = nullptr)
{
    if (adjoint)
        throw std::runtime_error("drt::hip::render: Dual numbers are forward mode: no adjoint image (a reverse-mode notion)");
    std::vector<double> v;
    const FlatScene<Dual<U>> flat = flatten_dual(scene, v);
    const drt_camera_desc cd = describe_dual(cam);
    std::vector<double> rgb, trgb;
    const Stats st = detail::tangent_call("drt::hip::render (Dual)", flat, cd, tracer.absorb(), tracer.min_bounces(), spp, v, rgb, trgb, opt);
    const std::size_t npix = cam.width() * cam.height();
    for (std::size_t i = 0; i < npix; ++i)
        for (int c = 0; c < 3; ++c)
            img[i][c] = Dual<U>(U(rgb[i * 3 + c]), U(trgb[i * 3 + c]));
    return st;
}

} } // namespace drt::hip
