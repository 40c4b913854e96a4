// kf_export.cpp — what leaves the orchestrator: point cloud and mesh with their PLY writers, the last frame's counters and the raw volume
// (the checkpoints: kf_checkpoint.cpp).  None of it runs during tracking.
#include "kf_internal.hpp"
#include <algorithm>
#include <cstring>
#include <fstream>

using namespace xs_host;

// reference :334-372
KinectFusionReconstruction::CPointCloud KinectFusionReconstruction::ExportPointCloud(int max_buffer) {
    CPointCloud res;
    if (max_buffer <= 0 || !tsdf_volume_d_ptr) return res;
    DeviceArray<float3> cloud_buffer, normal_buffer;
    cloud_buffer.create(max_buffer);
    normal_buffer.create(max_buffer);
    const int3 volume_res = make_int3(res3()[0], res3()[1], res3()[2]);
    // a rank of a sharded run reports the crossings of the planes it owns (the +z neighbour of its last
    // plane is in its halo); the single-GPU case is the whole volume
    const int z1 = std::min(zo1, volume_res.z - 1);
    PtrSz<float3> cloud; cloud.data = cloud_buffer.ptr(); cloud.size = (size_t)max_buffer;
    const size_t num_points = extractPoints(tsdf_volume_d_ptr->value(), tsdf_volume_d_ptr->weight(), tsdf_volume_d_ptr->grad(), volume_res,
                                            voxel_size, cloud, zs0, zo0, std::max(z1, zo0));
    if (num_points == 0) return res;
    cloud.size = num_points;
    PtrSz<float3> normal; normal.data = normal_buffer.ptr(); normal.size = num_points;
    extractNormals(tsdf_volume_d_ptr->value(), tsdf_volume_d_ptr->weight(), tsdf_volume_d_ptr->grad(), volume_res, voxel_size, cloud, normal,
                   zs0, zs1);
    res.positions.resize(3 * num_points);
    res.normals.resize(3 * num_points);
    hipSafeCall(hipMemcpy(res.positions.data(), cloud_buffer.ptr(), num_points * sizeof(float3), hipMemcpyDeviceToHost));
    hipSafeCall(hipMemcpy(res.normals.data(), normal_buffer.ptr(), num_points * sizeof(float3), hipMemcpyDeviceToHost));
    return res;
}
bool KinectFusionReconstruction::CPointCloud::exportPly(const std::string &filename) const {
    std::ofstream file_out{filename};
    if (!file_out.is_open()) return false;
    file_out << "ply\nformat ascii 1.0\ncomment Created by myself\nelement vertex " << size() << "\n";
    file_out << "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n";
    for (size_t i = 0; i < size(); ++i)
        file_out << positions[3 * i] << " " << positions[3 * i + 1] << " " << positions[3 * i + 2] << " " << normals[3 * i] << " "
                 << normals[3 * i + 1] << " " << normals[3 * i + 2] << "\n";
    return true;
}

KinectFusionReconstruction::CMesh KinectFusionReconstruction::ExportMesh(int min_weight) {
    CMesh m;
    if (!tsdf_volume_d_ptr) return m;
    if (sign_map_stale_) { RebuildSignMap(); sign_map_stale_ = false; }   // (the map must be a superset of the negative voxels)
    const int *res = res3();
    const bool seeded = csfd_seed_row >= 0 && csfd_seed_row < 4 && csfd_seed_col >= 0 && csfd_seed_col < 4;
    m.has_im = seeded;   // (also for an empty mesh: a rank without surface still says whether its vertices would carry derivatives)
    DeviceArray2D<float> value = tsdf_volume_d_ptr->value(), grad = tsdf_volume_d_ptr->grad();
    DeviceArray2D<int> weight = tsdf_volume_d_ptr->weight();
    // (TsdfVolume allocates the three arrays alike: one pitch)
    xs_mesh_opts o{};
    o.struct_bytes = sizeof(o);
    o.zs0 = zs0; o.zs1 = zs1;
    o.z0 = zo0; o.z1 = std::max(std::min(zo1, res[2] - 1), zo0);   // (as ExportPointCloud)
    o.min_weight = min_weight; o.want_normals = 1;
    o.signmap = sign_map_ptr(); o.signmap_shift = raycast_sign_map_shift;
    DeviceArray<unsigned char> ws;
    ws.create(xs_mesh_workspace_bytes(res, &o));
    const float *g = seeded ? grad.ptr(0) : nullptr;
    size_t nv = 0, nt = 0;
    int rc = xs_extract_mesh(value.ptr(0), weight.ptr(0), g, value.step(), res, voxel_size, &o, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0,
                             ws.ptr(), &nv, &nt, current_stream());
    if (rc == 0) return m;   // (nothing fits in no room only when there is nothing)
    if (rc != XS_MESH_OVER_CAPACITY) check_rc(rc, "mesh count");
    DeviceArray<float> verts, vim, normals;
    DeviceArray<unsigned long long> keys;
    DeviceArray<int> tris;
    verts.create(3 * nv); normals.create(3 * nv); keys.create(nv); tris.create(3 * std::max<size_t>(nt, 1));
    if (seeded) vim.create(3 * nv);
    size_t nv2 = 0, nt2 = 0;
    check_rc(xs_extract_mesh(value.ptr(0), weight.ptr(0), g, value.step(), res, voxel_size, &o, verts.ptr(), seeded ? vim.ptr() : nullptr,
                             normals.ptr(), keys.ptr(), nv, tris.ptr(), nt, ws.ptr(), &nv2, &nt2, current_stream()), "mesh");
    m.positions.resize(3 * nv); m.normals.resize(3 * nv); m.edge_keys.resize(nv); m.triangles.resize(3 * nt);
    hipSafeCall(hipMemcpy(m.positions.data(), verts.ptr(), 3 * nv * sizeof(float), hipMemcpyDeviceToHost));
    hipSafeCall(hipMemcpy(m.normals.data(), normals.ptr(), 3 * nv * sizeof(float), hipMemcpyDeviceToHost));
    hipSafeCall(hipMemcpy(m.edge_keys.data(), keys.ptr(), nv * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (nt) hipSafeCall(hipMemcpy(m.triangles.data(), tris.ptr(), 3 * nt * sizeof(int), hipMemcpyDeviceToHost));
    if (seeded) {
        m.vertex_im.resize(3 * nv);
        hipSafeCall(hipMemcpy(m.vertex_im.data(), vim.ptr(), 3 * nv * sizeof(float), hipMemcpyDeviceToHost));
    }
    return m;
}
bool KinectFusionReconstruction::CMesh::exportPly(const std::string &filename) const {
    std::ofstream f(filename, std::ios::binary);
    if (!f.is_open()) return false;
    const bool d = has_im;
    f << "ply\nformat binary_little_endian 1.0\nelement vertex " << vertices() << "\n";
    f << "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n";
    if (d) f << "property float dx\nproperty float dy\nproperty float dz\n";
    f << "element face " << faces() << "\nproperty list uchar int vertex_indices\nend_header\n";
    std::vector<float> row(d ? 9 : 6);   // (x86 / the hosts this builds for are little-endian: the floats go out as they are)
    for (size_t i = 0; i < vertices(); ++i) {
        for (int k = 0; k < 3; ++k) { row[k] = positions[3 * i + k]; row[3 + k] = normals[3 * i + k]; if (d) row[6 + k] = vertex_im[3 * i + k]; }
        f.write(reinterpret_cast<const char *>(row.data()), (std::streamsize)(row.size() * sizeof(float)));
    }
    char face[13];
    face[0] = 3;
    for (size_t t = 0; t < faces(); ++t) {
        std::memcpy(face + 1, &triangles[3 * t], 12);
        f.write(face, 13);
    }
    return (bool)f;
}

long long KinectFusionReconstruction::lastUpdatedVoxels() { return last_frame_counter(0); }
long long KinectFusionReconstruction::lastRaycastHits() { return last_frame_counter(1); }
long long KinectFusionReconstruction::last_frame_counter(int which) {
    if (counter_frame_ == 0) return 0;
    unsigned long long h[2] = {0, 0};
    synchronize();
    flush_pending_fold(current_stream());
    hipSafeCall(hipStreamSynchronize(current_stream()));
    hipSafeCall(hipMemcpy(h, counters_.ptr() + 2 * (size_t)((counter_frame_ - 1) % COUNTER_RING), sizeof(h), hipMemcpyDeviceToHost));
    return (long long)h[which];
}

// ---- the raw volume ------------------------------------------------------------------------
// reference :438-447 writes raw float32 values; here X*Y*Z of them (the reference's count uses
// res[2] twice)
void KinectFusionReconstruction::saveTSDFVolume(const std::string &tsdf_filename) {
    std::vector<float> tsdf;
    tsdf_volume_d_ptr->downloadTSDFWithoutGrad(tsdf);
    std::ofstream f(tsdf_filename, std::ios::binary);
    f.write(reinterpret_cast<const char *>(tsdf.data()), (std::streamsize)(tsdf.size() * sizeof(float)));
}
