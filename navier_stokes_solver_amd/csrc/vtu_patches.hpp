// vtu_patches.hpp — the VTU record of the C++ drivers (header-only, included by cli_main.cpp).
//
// What DataOut::write_vtu_with_pvtu_record leaves behind (NSSolverStationary.cpp:769-796, NSSolver.cpp:761-797): the
// rank's piece <name>_<counter>.<rank>.vtu and, on rank 0, the record <name>_<counter>.pvtu.  As deal.II's default
// build_patches() does, every cell is one patch with its own four vertices; point data `velocity` (3 components, z = 0),
// `pressure`, `partitioning`.  ASCII XML in exactly the layout of the Python writer (postprocess.write_vtu_patches):
// numbers as %.12g, one point per line.  The values come from nsk_state_get_patches: per cell (u_x, u_y) and p at the
// vertices (0,0), (1,0), (0,1), (1,1).  NSK_VTU_FORMAT=binary: the same piece as raw appended data (Record, below).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace vtu {

inline std::string counter_text(unsigned counter, int n_digits) {
  char buf[32];
  if (n_digits > 0) std::snprintf(buf, sizeof(buf), "%0*u", n_digits, counter);
  else std::snprintf(buf, sizeof(buf), "%u", counter);
  return buf;
}

// the derived arrays of the binary record, in file order; bit k of nsk_state_get_record_fields' mask
constexpr int kFields = 2;
inline const char *field_name(int k) { return k == 0 ? "vorticity" : "divergence"; }

// the record <name>_<cnt>.pvtu naming the pieces of all ranks; fields: the mask of the pieces' derived arrays
inline void write_pvtu(const std::filesystem::path &dir, const std::string &name, const std::string &cnt, int nranks,
                       unsigned fields = 0) {
  const std::string record = (dir / (name + "_" + cnt + ".pvtu")).string();
  std::FILE *f = std::fopen(record.c_str(), "w");
  if (!f) throw std::runtime_error("cannot write " + record);
  std::fprintf(f, "<?xml version=\"1.0\"?>\n<VTKFile type=\"PUnstructuredGrid\" version=\"0.1\" byte_order=\"LittleEndian\">\n"
                  "<PUnstructuredGrid GhostLevel=\"0\">\n<PPointData Scalars=\"scalars\">\n"
                  "<PDataArray type=\"Float64\" Name=\"velocity\" NumberOfComponents=\"3\" format=\"ascii\"/>\n"
                  "<PDataArray type=\"Float64\" Name=\"pressure\" format=\"ascii\"/>\n");
  for (int k = 0; k < kFields; ++k)
    if (fields >> k & 1u) std::fprintf(f, "<PDataArray type=\"Float64\" Name=\"%s\" format=\"ascii\"/>\n", field_name(k));
  std::fprintf(f, "<PDataArray type=\"Float64\" Name=\"partitioning\" format=\"ascii\"/>\n</PPointData>\n<PPoints>\n"
                  "<PDataArray type=\"Float64\" NumberOfComponents=\"3\"/>\n</PPoints>\n");
  for (int r = 0; r < nranks; ++r)
    std::fprintf(f, "%s<Piece Source=\"%s_%s.%d.vtu\"/>", r ? "\n" : "", name.c_str(), cnt.c_str(), r);
  std::fprintf(f, "\n</PUnstructuredGrid>\n</VTKFile>\n");
  if (std::fclose(f) != 0) throw std::runtime_error("cannot write " + record);
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
  if (rank == 0) write_pvtu(dir, name, cnt, nranks);
  return piece;
}

// The piece as VTK XML with raw appended data (postprocess.VtuRecord writes the same bytes from the same
// arrays): the XML header, then after <AppendedData encoding="raw"> and `_` the blocks — a UInt64 byte count and that many
// bytes each — points, velocity, pressure, [vorticity,] [divergence,] [partitioning,] connectivity, offsets, types.  The
// header is padded with blanks so that the first block starts at a multiple of 8 in the file.  Built once per run and rank
// with everything but velocity, pressure and the derived arrays filled in; a report fills vel3() / prs()
// (nsk_state_get_record) and field(k) (nsk_state_get_record_fields) and writes the image with one write.
class Record {
 public:
  // points: 3 doubles per point; rank < 0: no partitioning array; fields: mask of the derived arrays (0: the image without them)
  Record(int64_t n_points, const double *points, const std::vector<int32_t> &conn, const std::vector<int32_t> &offsets,
         const std::vector<uint8_t> &types, int rank, const char *declaration = "<?xml version=\"1.0\" ?>",
         const char *point_data = "Scalars=\"scalars\"", unsigned fields = 0)
      : n_points_(n_points), fields_(fields) {
    const size_t n = (size_t)n_points, m = offsets.size();
    if (types.size() != m) throw std::runtime_error("vtu::Record: offsets and types do not match");
    if (fields >> kFields) throw std::runtime_error("vtu::Record: unknown field");
    const bool part = rank >= 0;
    // blocks in file order: 0 points, 1 velocity, 2 pressure, 3 partitioning, 4 connectivity, 5 offsets, 6 types, 7 + k field k
    constexpr int NB = 7 + kFields;
    const int order[NB] = {0, 1, 2, 7, 8, 3, 4, 5, 6};
    const size_t bytes[NB] = {24 * n, 24 * n, 8 * n, 8 * n, 4 * conn.size(), 4 * m, m, 8 * n, 8 * n};
    const bool present[NB] = {true, true, true, part, true, true, true, (fields & 1u) != 0, (fields & 2u) != 0};
    size_t at[NB], pos = 0;
    for (int b : order) {
      at[b] = pos;
      if (present[b]) pos += 8 + bytes[b];
    }
    auto arr = [&](const char *type, const char *name, const char *extra, int b) {
      return std::string("<DataArray type=\"") + type + "\"" + (name ? std::string(" Name=\"") + name + "\"" : std::string()) +
             extra + " format=\"appended\" offset=\"" + std::to_string(at[b]) + "\"/>\n";
    };
    std::string head = std::string(declaration) +
                       "\n<VTKFile type=\"UnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\" "
                       "header_type=\"UInt64\">\n<UnstructuredGrid>\n<Piece NumberOfPoints=\"" +
                       std::to_string(n) + "\" NumberOfCells=\"" + std::to_string(m) + "\">\n<Points>\n" +
                       arr("Float64", nullptr, " NumberOfComponents=\"3\"", 0) + "</Points>\n<Cells>\n" +
                       arr("Int32", "connectivity", "", 4) + arr("Int32", "offsets", "", 5) + arr("UInt8", "types", "", 6) +
                       "</Cells>\n<PointData " + point_data + ">\n" +
                       arr("Float64", "velocity", " NumberOfComponents=\"3\"", 1) + arr("Float64", "pressure", "", 2) +
                       (present[7] ? arr("Float64", field_name(0), "", 7) : std::string()) +
                       (present[8] ? arr("Float64", field_name(1), "", 8) : std::string()) +
                       (part ? arr("Float64", "partitioning", "", 3) : std::string()) +
                       "</PointData>\n</Piece>\n</UnstructuredGrid>\n";
    const std::string opening = "<AppendedData encoding=\"raw\">\n_", closing = "\n</AppendedData>\n</VTKFile>\n";
    head += std::string((8 - (head.size() + opening.size()) % 8) % 8, ' ') + opening;
    const size_t start = head.size();
    // 8-byte words, so that vel3() and prs() are aligned doubles (start and every Float64 block are multiples of 8)
    size_ = start + pos + closing.size();
    image_.assign((size_ + 7) / 8, 0);
    char *im = reinterpret_cast<char *>(image_.data());
    std::memcpy(im, head.data(), start);
    std::memcpy(im + start + pos, closing.data(), closing.size());
    const std::vector<double> partv(part ? n : 0, (double)rank);
    const void *src[NB] = {points, nullptr, nullptr, partv.data(), conn.data(), offsets.data(), types.data(), nullptr, nullptr};
    for (int b = 0; b < NB; ++b) {
      if (!present[b]) continue;
      const uint64_t count = bytes[b];
      std::memcpy(im + start + at[b], &count, 8);
      if (src[b] && count) std::memcpy(im + start + at[b] + 8, src[b], count);
    }
    vel3_ = reinterpret_cast<double *>(im + start + at[1] + 8);
    prs_ = reinterpret_cast<double *>(im + start + at[2] + 8);
    for (int k = 0; k < kFields; ++k) field_[k] = present[7 + k] ? reinterpret_cast<double *>(im + start + at[7 + k] + 8) : nullptr;
  }
  Record(const Record &) = delete;
  Record &operator=(const Record &) = delete;

  int64_t n_points() const { return n_points_; }
  double *vel3() { return vel3_; }   // 3 per point: the file's velocity array
  double *prs() { return prs_; }     // 1 per point: the file's pressure array
  unsigned fields() const { return fields_; }
  double *field(int k) { return field_[k]; }   // 1 per point: the file's array field_name(k), or null
  const char *data() const { return reinterpret_cast<const char *>(image_.data()); }
  size_t size() const { return size_; }

  void write(const std::string &path) const {
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    const bool ok = std::fwrite(data(), 1, size_, f) == size_;
    if (std::fclose(f) != 0 || !ok) throw std::runtime_error("cannot write " + path);
  }
  // the files of write_patches: the piece <name>_<cnt>.<rank>.vtu and, on rank 0, the same .pvtu
  std::string write(const std::string &directory, const std::string &name, const std::string &cnt, int rank, int nranks) const {
    namespace fs = std::filesystem;
    const fs::path dir(directory.empty() ? "./" : directory);
    fs::create_directories(dir);
    const std::string piece = (dir / (name + "_" + cnt + "." + std::to_string(rank) + ".vtu")).string();
    write(piece);
    if (rank == 0) write_pvtu(dir, name, cnt, nranks, fields_);
    return piece;
  }

 private:
  int64_t n_points_;
  unsigned fields_ = 0;
  double *field_[kFields] = {nullptr, nullptr};
  size_t size_ = 0;
  std::vector<uint64_t> image_;
  double *vel3_ = nullptr, *prs_ = nullptr;
};

// The piece of the generated mesh's cells ij in file order with s = subdivisions in 1..4: per cell (s+1)^2 points
// ((i + k/s) hx, (j + l/s) hy, 0), pt = l (s+1) + k, and s^2 VTK_QUADs base + l (s+1) + k, +1, +(s+1)+1, +(s+1) — for s = 1
// the points and the `0 1 3 2` of write_patches.
inline std::unique_ptr<Record> quad_record(int64_t n_cells, const int32_t *ij, double hx, double hy, int s, int rank,
                                           unsigned fields = 0) {
  if (s < 1 || s > 4) throw std::runtime_error("vtu::quad_record: subdivisions outside 1..4");
  const int64_t ppc = (int64_t)(s + 1) * (s + 1), n_points = n_cells * ppc, n_quads = n_cells * s * s;
  std::vector<double> pts(3 * (size_t)n_points, 0.0);
  std::vector<int32_t> conn(4 * (size_t)n_quads), offs((size_t)n_quads);
  for (int64_t c = 0; c < n_cells; ++c) {
    for (int l = 0; l <= s; ++l)
      for (int k = 0; k <= s; ++k) {
        double *o = &pts[3 * (size_t)(c * ppc + l * (s + 1) + k)];
        o[0] = ((double)ij[2 * c] + (double)k / (double)s) * hx;
        o[1] = ((double)ij[2 * c + 1] + (double)l / (double)s) * hy;
      }
    for (int l = 0; l < s; ++l)
      for (int k = 0; k < s; ++k) {
        const int32_t first = (int32_t)(c * ppc + l * (s + 1) + k);
        int32_t *o = &conn[4 * (size_t)(c * s * s + l * s + k)];   // VTK_QUAD ordering
        o[0] = first; o[1] = first + 1; o[2] = first + s + 2; o[3] = first + s + 1;
      }
  }
  for (int64_t q = 0; q < n_quads; ++q) offs[(size_t)q] = (int32_t)(4 * (q + 1));
  return std::make_unique<Record>(n_points, pts.data(), conn, offs, std::vector<uint8_t>((size_t)n_quads, 9), rank,
                                  "<?xml version=\"1.0\" ?>", "Scalars=\"scalars\"", fields);
}

}  // namespace vtu
