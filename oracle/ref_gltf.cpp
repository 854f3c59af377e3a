// ref_gltf.cpp — builds the REFERENCE's own glTF parser (its vendored tinygltf + nlohmann json + stb_image) into
// oracle/_ref/libref_gltf.so, so that the tests can pin this repo's GLB loaders (host/scene_loader.cpp + host/json.h, rtamd/scenes.py)
// against exactly what the reference's Scene::Scene takes out of a file (tests/test_ref_gltf.py).
//
// TEST INFRASTRUCTURE ONLY. deps/tiny_gltf.cpp, deps/stb_image.cpp and deps/stb_image_write.cpp are compiled where they lie under $(REF)
// by `make -C oracle ref` (never copied into this repo); the recipe is a no-op where the reference tree is absent. This file holds only
// the wrapper: it loads a file as src/scene.cpp:56-62 does and hands back, as named flat arrays, every field that Scene::Scene, load_images,
// load_primitives and load_node read from the tinygltf::Model. It does no glm arithmetic: composing node matrices and the camera quaternion
// stay restated in the loaders and pinned by their own test. Each block names the src/scene.cpp lines it restates.
//
// The reference reads several things without looking (asserts are compiled out of its Release build). Where the file at hand would make
// it read past an end() iterator, index an array at -1 or read outside a buffer, the wrapper does NOT do that read: it records the case
// under "ub" (one line of text per case, with the src/scene.cpp line) and leaves the field out.
#include <cstdint>
#include <cstring>
#include <exception>
#include <map>
#include <string>
#include <vector>

#include "tiny_gltf.h"

namespace {

enum DType { F32 = 0, F64 = 1, I64 = 2, U32 = 3, U8 = 4 };

struct Array {
    int dtype;
    std::vector<uint8_t> bytes;
    uint64_t count;
};

struct Result {
    std::map<std::string, Array> arrays;
    std::string names; // '\n'-joined, in map order
    std::string ub;

    template <typename T> void put(const std::string& name, int dtype, const T* p, size_t n) {
        Array a;
        a.dtype = dtype, a.count = n;
        a.bytes.resize(n * sizeof(T));
        if (n) std::memcpy(a.bytes.data(), p, n * sizeof(T));
        arrays[name] = std::move(a);
    }
    void f32(const std::string& n, const std::vector<float>& v) { put(n, F32, v.data(), v.size()); }
    void f64(const std::string& n, const std::vector<double>& v) { put(n, F64, v.data(), v.size()); }
    void i64(const std::string& n, const std::vector<int64_t>& v) { put(n, I64, v.data(), v.size()); }
    void i64(const std::string& n, int64_t v) { put(n, I64, &v, 1); }
    void u32(const std::string& n, const std::vector<uint32_t>& v) { put(n, U32, v.data(), v.size()); }
    void text(const std::string& n, const std::string& s) { put(n, U8, (const uint8_t*)s.data(), s.size()); }
    void undefined(const std::string& what) { ub += what + "\n"; }
};

// The pointer-and-stride rule of src/scene.cpp:280-303 (POSITION), :307-328 (NORMAL), :332-353 (TEXCOORD_0):
//   base   = &buffers[view.buffer].data[accessor.byteOffset + view.byteOffset], read as const float*
//   stride = accessor.ByteStride(view) ? ByteStride(view) / sizeof(float) : packed width      (in floats)
//   element v = `width` floats at base[v * stride]; the count is the POSITION accessor's for all three (:289, :325, :351)
// The reference looks at neither componentType, type, normalized nor sparse: it reads floats whatever the accessor says.
bool read_attribute(const tinygltf::Model& m, Result& r, const tinygltf::Primitive& p, const char* semantic, int width, size_t count, std::vector<float>& out,
                    const std::string& where) {
    auto it = p.attributes.find(semantic);
    if (it == p.attributes.end()) {
        r.undefined(where + ": no " + semantic + ": attributes.find()->second on end() (src/scene.cpp:281/308/334)");
        return false;
    }
    if (it->second < 0 || (size_t)it->second >= m.accessors.size()) {
        r.undefined(where + ": " + semantic + " accessor index outside accessors[] (src/scene.cpp:281/308/334)");
        return false;
    }
    const tinygltf::Accessor& acc = m.accessors[(size_t)it->second];
    if (acc.bufferView < 0 || (size_t)acc.bufferView >= m.bufferViews.size()) {
        r.undefined(where + ": " + semantic + " accessor without a bufferView: bufferViews[-1] (src/scene.cpp:283/310/336)");
        return false;
    }
    const tinygltf::BufferView& view = m.bufferViews[(size_t)acc.bufferView];
    if (view.buffer < 0 || (size_t)view.buffer >= m.buffers.size()) {
        r.undefined(where + ": " + semantic + " view's buffer outside buffers[] (src/scene.cpp:285/312/338)");
        return false;
    }
    const std::vector<unsigned char>& data = m.buffers[(size_t)view.buffer].data;
    const size_t start = acc.byteOffset + view.byteOffset;
    const int bs = acc.ByteStride(view);
    const uint32_t stride = bs ? (uint32_t)((size_t)bs / sizeof(float)) : (uint32_t)width; // bs == -1 converts as the reference's does
    if (acc.componentType != TINYGLTF_COMPONENT_TYPE_FLOAT || acc.normalized || acc.sparse.isSparse ||
        acc.type != (width == 3 ? TINYGLTF_TYPE_VEC3 : TINYGLTF_TYPE_VEC2))
        r.undefined(where + ": " + semantic + " is not a plain float VEC" + std::to_string(width) + " accessor, and is read as one (src/scene.cpp:284/311/337)");
    if (count) {
        const size_t last = start + ((count - 1) * (size_t)stride + (size_t)width) * sizeof(float);
        if (bs < 0 || last > data.size()) {
            r.undefined(where + ": " + semantic + " read runs outside buffers[].data (src/scene.cpp:301-303/325-328/351-353)");
            return false;
        }
    }
    out.resize(count * (size_t)width);
    for (size_t v = 0; v < count; ++v) std::memcpy(&out[v * (size_t)width], data.data() + start + v * (size_t)stride * sizeof(float), sizeof(float) * (size_t)width);
    return true;
}

// Scene::load_node (src/scene.cpp:444-476): camera_node_index = node_index of every node visited that has a camera, in the order visited
// (a node before its children, children in order): the LAST one visited stays.
void visit(const tinygltf::Model& m, int node, int depth, std::vector<int64_t>& order, int& camera_node, bool& bad) {
    if (node < 0 || (size_t)node >= m.nodes.size() || depth > 256) {
        bad = true;
        return;
    }
    order.push_back(node);
    if (m.nodes[(size_t)node].camera != -1) camera_node = node; // :454-456
    for (int c : m.nodes[(size_t)node].children) visit(m, c, depth + 1, order, camera_node, bad); // :472-476
}

Result* load(const char* path) {
    Result* rp = new Result;
    Result& r = *rp;
    // ---- src/scene.cpp:56-62 ----
    tinygltf::Model m;
    tinygltf::TinyGLTF loader;
    std::string err, warn;
    loader.SetStoreOriginalJSONForExtrasAndExtensions(true);
    const bool ret = loader.LoadBinaryFromFile(&m, &err, &warn, path);
    r.i64("ret", ret ? 1 : 0);
    r.text("err", err);
    r.text("warn", warn);
    if (!ret || !err.empty()) return rp; // :68-70 throws

    // ---- Scene::load_images, src/scene.cpp:148-162: width, height and image.data() of every image, taken as RGBA8 ----
    r.i64("n_images", (int64_t)m.images.size());
    for (size_t i = 0; i < m.images.size(); ++i) {
        const tinygltf::Image& im = m.images[i];
        const std::string k = "image." + std::to_string(i) + ".";
        r.i64(k + "width", im.width), r.i64(k + "height", im.height), r.i64(k + "component", im.component), r.i64(k + "bits", im.bits);
        r.put(k + "bytes", U8, im.image.data(), im.image.size());
        if (im.as_is) r.undefined("image " + std::to_string(i) + ": as_is, no decoded pixels (src/scene.cpp:156)");
        if (im.bits != 8 || im.image.size() != (size_t)im.width * (size_t)im.height * 4)
            r.undefined("image " + std::to_string(i) + ": pixels are not width*height RGBA8, and are uploaded as that (src/scene.cpp:158-160)");
    }

    // ---- materials as Scene::load_primitives classifies them, src/scene.cpp:178-254 (there per primitive; the result depends on the material alone) ----
    r.i64("n_materials", (int64_t)m.materials.size());
    for (size_t i = 0; i < m.materials.size(); ++i) {
        const tinygltf::Material& gm = m.materials[i];
        const std::string k = "material." + std::to_string(i) + ".";
        const auto& pbr = gm.pbrMetallicRoughness;
        const std::vector<float> base = {(float)pbr.baseColorFactor[0], (float)pbr.baseColorFactor[1], (float)pbr.baseColorFactor[2]}; // :189-191
        float strength = 0.0f;                                                                                                       // :198-205
        if (auto e = gm.extensions.find("KHR_materials_emissive_strength"); e != gm.extensions.end())
            strength = (float)e->second.Get("emissiveStrength").GetNumberAsDouble();
        std::vector<float> emissive(3);
        for (int c = 0; c < 3; ++c) emissive[(size_t)c] = (float)gm.emissiveFactor[(size_t)c] * strength; // :193-196, :206
        auto ior_ext = gm.extensions.find("KHR_materials_ior");                                          // :208-210
        auto transmission_ext = gm.extensions.find("KHR_materials_transmission");
        int64_t cls, image = -1;
        float ior = 0.0f;
        if (ior_ext != gm.extensions.end() && transmission_ext != gm.extensions.end()) { // :212-218
            cls = 2;
            ior = (float)ior_ext->second.Get("ior").GetNumberAsDouble();
        } else {
            cls = pbr.metallicFactor > 0.01f ? 1 : 0; // :219, the double factor against the float literal
            if (pbr.baseColorTexture.index > -1) {    // :221-227, :241-247
                const uint32_t texture_index = (uint32_t)pbr.baseColorTexture.index;
                if (texture_index >= m.textures.size()) {
                    r.undefined("material " + std::to_string(i) + ": baseColorTexture.index outside textures[] (src/scene.cpp:224/244)");
                } else {
                    const int src = m.textures[texture_index].source;
                    if (src < 0 || (size_t)src >= m.images.size()) r.undefined("material " + std::to_string(i) + ": texture source outside images[] (src/scene.cpp:226/246)");
                    else image = src;
                }
            }
        }
        r.i64(k + "class", cls), r.i64(k + "image", image);
        r.f32(k + "ior", {ior}), r.f32(k + "base_color", base), r.f32(k + "emissive", emissive), r.f32(k + "roughness", {(float)pbr.roughnessFactor}); // :231
    }

    // ---- Scene::load_primitives, src/scene.cpp:164-402 ----
    std::vector<int64_t> prim_count;
    for (size_t mi = 0; mi < m.meshes.size(); ++mi) {
        prim_count.push_back((int64_t)m.meshes[mi].primitives.size());
        for (size_t pi = 0; pi < m.meshes[mi].primitives.size(); ++pi) {
            const tinygltf::Primitive& p = m.meshes[mi].primitives[pi];
            const std::string where = "mesh " + std::to_string(mi) + " primitive " + std::to_string(pi);
            const std::string k = "prim." + std::to_string(mi) + "." + std::to_string(pi) + ".";
            r.i64(k + "material", p.material);
            if (p.material < 0 || (size_t)p.material >= m.materials.size()) r.undefined(where + ": no material: materials[-1] (src/scene.cpp:176-179)");
            size_t vertex_count = 0;
            if (auto it = p.attributes.find("POSITION"); it != p.attributes.end() && it->second >= 0 && (size_t)it->second < m.accessors.size())
                vertex_count = m.accessors[(size_t)it->second].count; // :289, :296
            std::vector<float> pos, nrm, uv;
            if (read_attribute(m, r, p, "POSITION", 3, vertex_count, pos, where)) r.f32(k + "positions", pos);
            if (read_attribute(m, r, p, "NORMAL", 3, vertex_count, nrm, where)) r.f32(k + "normals", nrm);
            if (read_attribute(m, r, p, "TEXCOORD_0", 2, vertex_count, uv, where)) r.f32(k + "uvs", uv);
            // indices, :356-402: accessors[indices > -1 ? indices : 0], data at accessor.byteOffset + view.byteOffset, read PACKED in the
            // accessor's component type (the view's byteStride is not looked at) and widened to uint32
            if (p.indices < 0) r.undefined(where + ": no indices: accessor 0 is read as the index list (src/scene.cpp:356-358)");
            const size_t ia = p.indices > -1 ? (size_t)p.indices : 0;
            if (p.indices < 0 || ia >= m.accessors.size()) continue;
            const tinygltf::Accessor& acc = m.accessors[ia];
            if (acc.bufferView < 0 || (size_t)acc.bufferView >= m.bufferViews.size()) {
                r.undefined(where + ": index accessor without a bufferView (src/scene.cpp:359-360)");
                continue;
            }
            const tinygltf::BufferView& view = m.bufferViews[(size_t)acc.bufferView];
            if (view.buffer < 0 || (size_t)view.buffer >= m.buffers.size()) continue;
            const std::vector<unsigned char>& data = m.buffers[(size_t)view.buffer].data;
            const size_t start = acc.byteOffset + view.byteOffset;
            size_t width = 0;
            switch (acc.componentType) {
            case TINYGLTF_PARAMETER_TYPE_UNSIGNED_INT: width = 4; break;   // :375-381
            case TINYGLTF_PARAMETER_TYPE_UNSIGNED_SHORT: width = 2; break; // :382-388
            case TINYGLTF_PARAMETER_TYPE_UNSIGNED_BYTE: width = 1; break;  // :389-395
            default: r.undefined(where + ": index component type not supported, the indices stay unwritten (src/scene.cpp:396-401)"); continue;
            }
            if (start + acc.count * width > data.size()) {
                r.undefined(where + ": index read runs outside buffers[].data (src/scene.cpp:363-366)");
                continue;
            }
            if (acc.count % 3) r.undefined(where + ": index count is no multiple of 3 (src/scene.cpp:368)");
            std::vector<uint32_t> idx(acc.count);
            for (size_t i = 0; i < acc.count; ++i) {
                const unsigned char* s = data.data() + start + i * width;
                if (width == 4) std::memcpy(&idx[i], s, 4);
                else if (width == 2) { uint16_t t; std::memcpy(&t, s, 2); idx[i] = t; }
                else idx[i] = *s;
            }
            r.u32(k + "indices", idx);
        }
    }
    r.i64("mesh_primitives", prim_count);

    // ---- the scene the reference picks and its sky extras, src/scene.cpp:77-94 ----
    r.i64("default_scene", m.defaultScene);
    const size_t si = (size_t)(m.defaultScene > -1 ? m.defaultScene : 0);
    r.i64("scene", (int64_t)si);
    if (si >= m.scenes.size()) {
        r.undefined("the picked scene is outside scenes[] (src/scene.cpp:77-78)");
        return rp;
    }
    const tinygltf::Scene& scene = m.scenes[si];
    if (auto sky = scene.extras.Get("sky_color"); sky.IsArray() && sky.Size() == 3) // :80-86
        r.f32("sky_color", {(float)sky.Get(0).GetNumberAsDouble(), (float)sky.Get(1).GetNumberAsDouble(), (float)sky.Get(2).GetNumberAsDouble()});
    if (auto s = scene.extras.Get("sky_strength"); s.IsNumber()) r.f32("sky_strength", {(float)s.GetNumberAsDouble()}); // :90-92
    r.i64("scene_nodes", std::vector<int64_t>(scene.nodes.begin(), scene.nodes.end()));

    // ---- nodes: the raw fields Scene::load_node reads, src/scene.cpp:450-480 (it takes T / R / S / matrix only at sizes 3 / 4 / 3 / 16) ----
    r.i64("n_nodes", (int64_t)m.nodes.size());
    for (size_t i = 0; i < m.nodes.size(); ++i) {
        const tinygltf::Node& n = m.nodes[i];
        const std::string k = "node." + std::to_string(i) + ".";
        r.f64(k + "matrix", n.matrix), r.f64(k + "translation", n.translation), r.f64(k + "rotation", n.rotation), r.f64(k + "scale", n.scale);
        r.i64(k + "children", std::vector<int64_t>(n.children.begin(), n.children.end()));
        r.i64(k + "mesh", n.mesh), r.i64(k + "camera", n.camera);
        if (n.mesh != -1 && (n.mesh < 0 || (size_t)n.mesh >= m.meshes.size())) r.undefined("node " + std::to_string(i) + ": mesh outside meshes[] (src/scene.cpp:480-481)");
    }

    // ---- the camera node, src/scene.cpp:96-99, :454-456 and :109-127 ----
    std::vector<int64_t> order;
    int camera_node = -1; // src/scene.hpp:70
    bool bad = false;
    for (int root : scene.nodes) visit(m, root, 0, order, camera_node, bad);
    if (bad) r.undefined("a scene or child node index outside nodes[], or a hierarchy deeper than 256 (src/scene.cpp:450-451)");
    r.i64("visit_order", order);
    r.i64("camera_node_index", camera_node);
    // `if (this->camera_node_index)` (:109) tests an int that starts at -1: a camera on node 0 is NOT taken (the members keep what main() wrote
    // before), and NO camera node at all (-1) enters the block and indexes nodes[-1]
    if (camera_node == -1) {
        r.undefined("no camera node: camera_node_index stays -1, which is true, and nodes[-1] is read (src/scene.cpp:109-111)");
    } else if (camera_node != 0) {
        const int cam = m.nodes[(size_t)camera_node].camera;
        if (cam < 0 || (size_t)cam >= m.cameras.size()) r.undefined("the camera node's camera is outside cameras[] (src/scene.cpp:123)");
        else r.f32("camera_yfov", {(float)m.cameras[(size_t)cam].perspective.yfov}); // :123, float yfov = (double)
    }
    return rp;
}

} // namespace

extern "C" {

void* ref_gltf_load(const char* path) {
    Result* r;
    try {
        r = load(path);
    } catch (const std::exception& e) { // (the reference would end on the uncaught exception)
        r = new Result;
        r->i64("ret", 0), r->text("err", std::string("exception: ") + e.what()), r->text("warn", "");
    }
    r->text("ub", r->ub);
    for (const auto& kv : r->arrays) r->names += kv.first + "\n";
    return r;
}
const char* ref_gltf_names(void* h) { return ((Result*)h)->names.c_str(); }
// dtype: 0 float32, 1 float64, 2 int64, 3 uint32, 4 uint8
const void* ref_gltf_array(void* h, const char* name, int* dtype, uint64_t* count) {
    Result* r = (Result*)h;
    auto it = r->arrays.find(name);
    if (it == r->arrays.end()) return nullptr;
    *dtype = it->second.dtype, *count = it->second.count;
    return it->second.bytes.data();
}
void ref_gltf_free(void* h) { delete (Result*)h; }
}
