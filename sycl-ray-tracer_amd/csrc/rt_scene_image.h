// rt_scene_image.h — the device image of a built HostScene: the form its arrays take in device memory, the way back, the scalars of SceneDev.
// rt_scene_create_ex (rt_abi.hip) writes it, rt_scene_update rewrites it in place and sync_host_copy reads it back (rt_update.hip). Host code.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "scene_build.h"

namespace rt {

// The node array: child words as byte offsets (rt_types.h). A tree of more nodes (33 M: ~130 M triangles) has no device form.
constexpr size_t kMaxDeviceNodes = 0x7FFFFFFF / sizeof(BvhNode);
inline std::vector<BvhNode> device_nodes(const std::vector<BvhNode>& host) {
    std::vector<BvhNode> dn(host);
    for (BvhNode& n : dn)
        for (int k = 0; k < 4; ++k) n.child[k] = (int32_t)device_child_word(n.child[k]);
    return dn;
}
inline void host_nodes(std::vector<BvhNode>& nodes) { // in place, the inverse
    for (BvhNode& n : nodes)
        for (int k = 0; k < 4; ++k) n.child[k] = host_child_word((uint32_t)n.child[k]);
}

// The leaf records: a TriRec's ten live dwords at a kTriBytes stride, and a zero tail (the whole-leaf step reads 80 bytes at every leaf).
constexpr size_t kTriTailBytes = 48;
static_assert(kTriBytes + kTriTailBytes >= 80 && kTriBytes <= sizeof(TriRec), "a last leaf of one record is read as five 16-byte loads too");
inline size_t packed_tri_bytes(size_t n_records) { return n_records * kTriBytes + kTriTailBytes; }
inline std::vector<uint8_t> pack_tris(const std::vector<TriRec>& tris) {
    std::vector<uint8_t> packed(packed_tri_bytes(tris.size()), 0);
    for (size_t r = 0; r < tris.size(); ++r) std::memcpy(packed.data() + r * kTriBytes, &tris[r], kTriBytes);
    return packed;
}
inline void unpack_tris(const std::vector<uint8_t>& packed, std::vector<TriRec>& tris) { // (a record's two padding words stay)
    for (size_t r = 0; r < tris.size(); ++r) std::memcpy(&tris[r], packed.data() + r * kTriBytes, kTriBytes);
}

// Every scalar of SceneDev. LDS staging (rt_device.h: ShadeTables): the head of the distinct-matrix and material tables, layers in 16 bits.
inline void scene_scalars(const HostScene& hs, SceneDev& dev) {
    dev.n_nodes = (uint32_t)hs.nodes.size();
    dev.n_tris = (uint32_t)(hs.wverts.size() / 9);
    std::memcpy(dev.sky, hs.sky, 12);
    dev.packed_mat = hs.packed_mat ? 1u : 0u;
    const bool stage = hs.packed_mat && hs.n_layers <= 65536u;
    dev.lds_nm = stage ? (uint32_t)std::min<size_t>(hs.inst.size(), kLdsNm) : 0u;
    dev.lds_mats = stage ? (uint32_t)std::min<size_t>(hs.mats.size(), kLdsMats) : 0u;
    for (int a = 0; a < 3; ++a) { // the ray re-ordering cells: 0..4 per axis over the scene's bounds
        const float ext = hs.bounds_hi[a] - hs.bounds_lo[a];
        dev.cell_lo[a] = hs.bounds_lo[a];
        dev.cell_scale[a] = ext > 0.0f && std::isfinite(ext) ? 4.0f / ext : 0.0f;
    }
}

} // namespace rt
