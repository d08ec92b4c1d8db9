// vtu_patches.hpp — the VTU record of the C++ drivers (header-only, included by cli_main.cpp).
//
// What DataOut::write_vtu_with_pvtu_record leaves behind (NSSolverStationary.cpp:769-796, NSSolver.cpp:761-797): the
// rank's piece <name>_<counter>.<rank>.vtu and, on rank 0, the record <name>_<counter>.pvtu.  As deal.II's default
// build_patches() does, every cell is one patch with its own four vertices; point data `velocity` (3 components, z = 0),
// `pressure`, `partitioning`.  ASCII XML in exactly the layout of the Python writer (postprocess.write_vtu_patches):
// numbers as %.12g, one point per line.  The values come from nsk_state_get_patches: per cell (u_x, u_y) and p at the
// vertices (0,0), (1,0), (0,1), (1,1).
#pragma once
#include <cstdint>
#include <cstdio>
#include <filesystem>
#include <stdexcept>
#include <string>

namespace vtu {

inline std::string counter_text(unsigned counter, int n_digits) {
  char buf[32];
  if (n_digits > 0) std::snprintf(buf, sizeof(buf), "%0*u", n_digits, counter);
  else std::snprintf(buf, sizeof(buf), "%u", counter);
  return buf;
}

// ij: (i, j) per cell; vel: 8 doubles per cell; prs: 4 per cell.  Returns the path of the piece.
inline std::string write_patches(const std::string &directory, const std::string &name, const std::string &cnt,
                                 int64_t n_cells, const int32_t *ij, double hx, double hy, const double *vel,
                                 const double *prs, int rank, int nranks) {
  namespace fs = std::filesystem;
  const fs::path dir(directory.empty() ? "./" : directory);
  fs::create_directories(dir);
  const std::string piece = (dir / (name + "_" + cnt + "." + std::to_string(rank) + ".vtu")).string();
  std::FILE *f = std::fopen(piece.c_str(), "w");
  if (!f) throw std::runtime_error("cannot write " + piece);
  const long long n_pts = 4 * (long long)n_cells;
  const int da[4] = {0, 1, 0, 1}, db[4] = {0, 0, 1, 1};   // deal.II vertex order of a patch
  std::fprintf(f, "<?xml version=\"1.0\" ?>\n<VTKFile type=\"UnstructuredGrid\" version=\"0.1\" byte_order=\"LittleEndian\">\n"
                  "<UnstructuredGrid>\n<Piece NumberOfPoints=\"%lld\" NumberOfCells=\"%lld\">\n<Points>\n"
                  "<DataArray type=\"Float64\" NumberOfComponents=\"3\" format=\"ascii\">\n", n_pts, (long long)n_cells);
  for (long long p = 0; p < n_pts; ++p)
    std::fprintf(f, "%s%.12g %.12g 0", p ? "\n" : "", (double)(ij[2 * (p / 4)] + da[p % 4]) * hx,
                 (double)(ij[2 * (p / 4) + 1] + db[p % 4]) * hy);
  std::fprintf(f, "\n</DataArray>\n</Points>\n<Cells>\n<DataArray type=\"Int32\" Name=\"connectivity\" format=\"ascii\">\n");
  for (long long c = 0; c < n_cells; ++c)   // VTK_QUAD ordering
    std::fprintf(f, "%s%lld %lld %lld %lld", c ? "\n" : "", 4 * c, 4 * c + 1, 4 * c + 3, 4 * c + 2);
  std::fprintf(f, "\n</DataArray>\n<DataArray type=\"Int32\" Name=\"offsets\" format=\"ascii\">\n");
  for (long long c = 0; c < n_cells; ++c) std::fprintf(f, "%s%lld", c ? " " : "", 4 * (c + 1));
  std::fprintf(f, "\n</DataArray>\n<DataArray type=\"UInt8\" Name=\"types\" format=\"ascii\">\n");
  for (long long c = 0; c < n_cells; ++c) std::fprintf(f, "%s9", c ? " " : "");
  std::fprintf(f, "\n</DataArray>\n</Cells>\n<PointData Scalars=\"scalars\">\n"
                  "<DataArray type=\"Float64\" Name=\"velocity\" NumberOfComponents=\"3\" format=\"ascii\">\n");
  for (long long p = 0; p < n_pts; ++p) std::fprintf(f, "%s%.12g %.12g 0", p ? "\n" : "", vel[2 * p], vel[2 * p + 1]);
  std::fprintf(f, "\n</DataArray>\n<DataArray type=\"Float64\" Name=\"pressure\" format=\"ascii\">\n");
  for (long long p = 0; p < n_pts; ++p) std::fprintf(f, "%s%.12g", p ? "\n" : "", prs[p]);
  std::fprintf(f, "\n</DataArray>\n<DataArray type=\"Float64\" Name=\"partitioning\" format=\"ascii\">\n");
  for (long long p = 0; p < n_pts; ++p) std::fprintf(f, "%s%d.0", p ? " " : "", rank);
  std::fprintf(f, "\n</DataArray>\n</PointData>\n</Piece>\n</UnstructuredGrid>\n</VTKFile>\n");
  if (std::fclose(f) != 0) throw std::runtime_error("cannot write " + piece);
  if (rank != 0) return piece;
  const std::string record = (dir / (name + "_" + cnt + ".pvtu")).string();
  f = std::fopen(record.c_str(), "w");
  if (!f) throw std::runtime_error("cannot write " + record);
  std::fprintf(f, "<?xml version=\"1.0\"?>\n<VTKFile type=\"PUnstructuredGrid\" version=\"0.1\" byte_order=\"LittleEndian\">\n"
                  "<PUnstructuredGrid GhostLevel=\"0\">\n<PPointData Scalars=\"scalars\">\n"
                  "<PDataArray type=\"Float64\" Name=\"velocity\" NumberOfComponents=\"3\" format=\"ascii\"/>\n"
                  "<PDataArray type=\"Float64\" Name=\"pressure\" format=\"ascii\"/>\n"
                  "<PDataArray type=\"Float64\" Name=\"partitioning\" format=\"ascii\"/>\n</PPointData>\n<PPoints>\n"
                  "<PDataArray type=\"Float64\" NumberOfComponents=\"3\"/>\n</PPoints>\n");
  for (int r = 0; r < nranks; ++r)
    std::fprintf(f, "%s<Piece Source=\"%s_%s.%d.vtu\"/>", r ? "\n" : "", name.c_str(), cnt.c_str(), r);
  std::fprintf(f, "\n</PUnstructuredGrid>\n</VTKFile>\n");
  if (std::fclose(f) != 0) throw std::runtime_error("cannot write " + record);
  return piece;
}

}  // namespace vtu
