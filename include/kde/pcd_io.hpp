// kde/pcd_io.hpp — header-only writer of PCD v0.7 files for the XYZRGB records of kde::PointCloudXYZRGB (kde_cloud_point):
// what pcl::io::savePCDFile writes for the pcl::PointCloud<pcl::PointXYZRGB> main.cpp:211-300 builds.  No PCL, no HIP: the
// records are host memory (PointCloudXYZRGB::points_Host).  The Python writer (pcdio.write_pcd) produces the same bytes.
//
//   header   # .PCD v0.7 - Point Cloud Data file format / VERSION 0.7 / FIELDS x y z rgb / SIZE 4 4 4 4 / TYPE F F F U /
//            COUNT 1 1 1 1 / WIDTH w / HEIGHT h / VIEWPOINT 0 0 0 1 0 0 0 / POINTS w*h / DATA binary|ascii
//   dense    writePcd(path, records, count)            WIDTH count, HEIGHT 1
//   organised writePcd(path, records, W * H, W, H)     WIDTH W, HEIGHT H
//   binary   the record array as it is in memory (little endian); ascii: `x y z rgb` per line, the floats with nine
//            significant digits, a NaN as `nan`
#ifndef KDE_PCD_IO_HPP
#define KDE_PCD_IO_HPP

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../kde_hip.h"

namespace kde {

inline std::string pcdHeader(size_t width, size_t height, bool binary)
{
    std::string h = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n";
    h += "WIDTH " + std::to_string(width) + "\nHEIGHT " + std::to_string(height) + "\nVIEWPOINT 0 0 0 1 0 0 0\n";
    h += "POINTS " + std::to_string(width * height) + "\nDATA " + (binary ? "binary" : "ascii") + "\n";
    return h;
}

// false when width * height != count or the file cannot be written
inline bool writePcd(const char* path, const kde_cloud_point* points, size_t count, size_t width, size_t height, bool binary = true)
{
    if (height < 1 || width * height != count || (count && !points)) return false;
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const std::string h = pcdHeader(width, height, binary);
    bool ok = std::fwrite(h.data(), 1, h.size(), f) == h.size();
    if (binary) {
        ok = ok && (count == 0 || std::fwrite(points, sizeof(kde_cloud_point), count, f) == count);
    } else {
        for (size_t i = 0; ok && i < count; ++i) {
            const float v[3] = {points[i].x, points[i].y, points[i].z};
            for (int k = 0; k < 3 && ok; ++k) ok = (v[k] != v[k] ? std::fprintf(f, "nan ") : std::fprintf(f, "%.9g ", (double)v[k])) > 0;
            ok = ok && std::fprintf(f, "%u\n", (unsigned)points[i].rgb) > 0;
        }
    }
    return (std::fclose(f) == 0) && ok;
}

// a dense cloud: WIDTH count, HEIGHT 1
inline bool writePcd(const char* path, const kde_cloud_point* points, size_t count, bool binary = true)
{
    return writePcd(path, points, count, count, 1, binary);
}

}  // namespace kde

#endif  // KDE_PCD_IO_HPP
