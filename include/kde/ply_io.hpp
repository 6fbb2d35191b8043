// kde/ply_io.hpp — header-only writer of PLY 1.0 files for the meshes of kde::OrganizedMesh: the vertex records
// (kde_cloud_point, the cloud of main.cpp:211-300) and the triangles (kde_mesh_triangle).  No HIP: the records are host memory
// (OrganizedMesh::vertices_Host / triangles_Host).  The Python writer (plyio.write_ply) produces the same bytes.
//
//   header   ply / format binary_little_endian 1.0 | ascii 1.0 / element vertex N / property float x, y, z /
//            property uchar red, green, blue / element face M / property list uchar int vertex_indices / end_header
//   binary   N records of 15 bytes (three floats, r, g, b), then M records of 13 bytes (the count 3, three int32)
//   ascii    `x y z r g b` per vertex, the floats with nine significant digits, a NaN as `nan`; `3 i j k` per face
#ifndef KDE_PLY_IO_HPP
#define KDE_PLY_IO_HPP

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../kde_hip.h"

namespace kde {

inline std::string plyHeader(size_t vertices, size_t faces, bool binary)
{
    std::string h = "ply\nformat ";
    h += binary ? "binary_little_endian" : "ascii";
    h += " 1.0\nelement vertex " + std::to_string(vertices) + "\nproperty float x\nproperty float y\nproperty float z\n";
    h += "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face " + std::to_string(faces) + "\n";
    h += "property list uchar int vertex_indices\nend_header\n";
    return h;
}

// false when a triangle names a vertex that is not there or the file cannot be written
inline bool writePly(const char* path, const kde_cloud_point* vertices, size_t vertex_count, const kde_mesh_triangle* triangles,
                     size_t triangle_count, bool binary = true)
{
    if ((vertex_count && !vertices) || (triangle_count && !triangles)) return false;
    for (size_t i = 0; i < triangle_count; ++i)
        if (triangles[i].v0 >= vertex_count || triangles[i].v1 >= vertex_count || triangles[i].v2 >= vertex_count) return false;
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const std::string h = plyHeader(vertex_count, triangle_count, binary);
    bool ok = std::fwrite(h.data(), 1, h.size(), f) == h.size();
    if (binary) {
        std::vector<unsigned char> buf;
        buf.resize(15 * vertex_count + 13 * triangle_count);
        unsigned char* p = buf.data();
        for (size_t i = 0; i < vertex_count; ++i, p += 15) {
            std::memcpy(p, &vertices[i], 12);                   // x, y, z as they are in memory (little endian)
            p[12] = (unsigned char)(vertices[i].rgb >> 16);
            p[13] = (unsigned char)(vertices[i].rgb >> 8);
            p[14] = (unsigned char)vertices[i].rgb;
        }
        for (size_t i = 0; i < triangle_count; ++i, p += 13) {
            p[0] = 3;
            std::memcpy(p + 1, &triangles[i], 12);
        }
        ok = ok && (buf.empty() || std::fwrite(buf.data(), 1, buf.size(), f) == buf.size());
    } else {
        for (size_t i = 0; ok && i < vertex_count; ++i) {
            const float v[3] = {vertices[i].x, vertices[i].y, vertices[i].z};
            for (int k = 0; k < 3 && ok; ++k) ok = (v[k] != v[k] ? std::fprintf(f, "nan ") : std::fprintf(f, "%.9g ", (double)v[k])) > 0;
            const unsigned c = (unsigned)vertices[i].rgb;
            ok = ok && std::fprintf(f, "%u %u %u\n", (c >> 16) & 255u, (c >> 8) & 255u, c & 255u) > 0;
        }
        for (size_t i = 0; ok && i < triangle_count; ++i)
            ok = std::fprintf(f, "3 %u %u %u\n", (unsigned)triangles[i].v0, (unsigned)triangles[i].v1, (unsigned)triangles[i].v2) > 0;
    }
    return (std::fclose(f) == 0) && ok;
}

}  // namespace kde

#endif  // KDE_PLY_IO_HPP
