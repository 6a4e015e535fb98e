// api_field.cpp — the C ABI's distance field of the raster map (include/f110qp.h, rules D1 to D4):
// f110qp_grid_distance_dev, f110qp_grid_inflate_dev and f110qp_grid_lookup_dev on the device, f110qp_grid_field and
// f110qp_wall_distance on host pointers. Host-side responsibilities only: the argument rules (every one answers
// before the first HIP call), the launches, and the synchronous calls' own staging. No C++ exception crosses this
// boundary.
#include "api_common.h"

namespace {

// The map's own rules (grid_params, with `grid` whichever array the call reads the cells of) and the field's
// limit on top: with both sides at most 32,768 every squared cell distance is below INT_MAX.
int field_params(const f110qp_grid_config* gc, const void* grid, f110qp::GridParams* Gr) {
  if (const int rv = grid_params(gc, 0, grid, Gr)) return rv;
  if (gc->width > F110QP_FIELD_MAX_SIDE || gc->height > F110QP_FIELD_MAX_SIDE)
    return fail(F110QP_ERR_INVALID, "grid width and height must be <= 32768 for the distance field");
  return F110QP_OK;
}

bool has_cells(const f110qp::GridParams& Gr) { return Gr.W > 0 && Gr.H > 0; }

const char* check_radius(double radius) {
  if (!(radius >= 0.0) || !std::isfinite(radius)) return "radius must be >= 0 and finite";
  return nullptr;
}

// batch and rows as f110qp_progress_dev, then the lookup's pointers.
const char* check_lookup(int batch, int rows, const double* x, const double* dist, const int* nearest,
                         const int* cell) {
  if (batch < 1) return "batch must be >= 1";
  if (rows < 1) return "rows must be >= 1";
  if ((long long)rows * batch > (1ll << 30)) return "rows x batch too large";
  if (!x || !dist) return "x/dist must be non-NULL";
  if ((nearest == nullptr) != (cell == nullptr)) return "nearest and cell must be given together or both be NULL";
  return nullptr;
}

// One staged call's copies on the null stream, the first error kept.
struct Copies {
  hipError_t e = hipSuccess;
  void up(void* d, const void* host, size_t bytes) {
    if (host && bytes && e == hipSuccess) e = hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, nullptr);
  }
  void back(void* host, const void* d, size_t bytes) {
    if (host && bytes && e == hipSuccess) e = hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, nullptr);
  }
};

size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }

}  // namespace

extern "C" {

int f110qp_grid_distance_dev(const f110qp_grid_config* gc, const unsigned char* grid, int* d2, int* nearest,
                             int* work, void* stream) {
  f110qp::GridParams Gr;
  if (const int rv = field_params(gc, grid, &Gr)) return rv;
  if (!has_cells(Gr)) return F110QP_OK;
  if (!d2 || !work) return fail(F110QP_ERR_INVALID, "d2/work must be non-NULL");
  const hipError_t e = f110qp::launch_grid_distance(Gr.W, Gr.H, grid, d2, nearest, work, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "grid distance launch");
  return F110QP_OK;
}

int f110qp_grid_inflate_dev(const f110qp_grid_config* gc, const int* d2, double radius, unsigned char* out,
                            void* stream) {
  f110qp::GridParams Gr;
  if (const int rv = field_params(gc, gc, &Gr)) return rv;  // the cells are d2's: checked below
  if (const char* m = check_radius(radius)) return fail(F110QP_ERR_INVALID, m);
  if (!has_cells(Gr)) return F110QP_OK;
  if (!d2 || !out) return fail(F110QP_ERR_INVALID, "d2/out must be non-NULL");
  const hipError_t e = f110qp::launch_grid_inflate(Gr.W, Gr.H, Gr.res, d2, radius, out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "grid inflate launch");
  return F110QP_OK;
}

int f110qp_grid_lookup_dev(const f110qp_grid_config* gc, const int* d2, const int* nearest, int batch, int rows,
                           const double* x, double* dist, int* cell, void* stream) {
  f110qp::GridParams Gr;
  if (const int rv = field_params(gc, gc, &Gr)) return rv;
  if (const char* m = check_lookup(batch, rows, x, dist, nearest, cell)) return fail(F110QP_ERR_INVALID, m);
  if (has_cells(Gr) && !d2) return fail(F110QP_ERR_INVALID, "width * height > 0 needs d2");
  const hipError_t e = f110qp::launch_grid_lookup(Gr, d2, nearest, batch, rows, x, dist, cell, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "grid lookup launch");
  return F110QP_OK;
}

int f110qp_grid_field(const f110qp_grid_config* gc, const unsigned char* grid, double radius, int* d2, int* nearest,
                      unsigned char* inflated) {
  f110qp::GridParams Gr;
  if (const int rv = field_params(gc, grid, &Gr)) return rv;
  if (inflated)
    if (const char* m = check_radius(radius)) return fail(F110QP_ERR_INVALID, m);
  if (!has_cells(Gr)) return F110QP_OK;
  if (!d2) return fail(F110QP_ERR_INVALID, "d2 must be non-NULL");
  const size_t n = (size_t)Gr.W * (size_t)Gr.H;

  // one device buffer, freed with `dev` on every way out: d2, nearest, work, then the two byte maps
  DevBuf dev;
  hipError_t e = dev.ensure(3 * n * sizeof(int) + 2 * round8(n));
  if (e != hipSuccess) return hip_fail(e, "field staging allocation");
  int* dd2 = (int*)dev.p;
  int *dnear = dd2 + n, *dwork = dnear + n;
  unsigned char* dgrid = (unsigned char*)(dwork + n);
  unsigned char* dout = dgrid + round8(n);
  Copies cp;
  cp.up(dgrid, grid, n);
  if (cp.e != hipSuccess) {
    (void)hipStreamSynchronize(nullptr);
    return hip_fail(cp.e, "field H2D");
  }
  int rv = f110qp_grid_distance_dev(gc, dgrid, dd2, nearest ? dnear : nullptr, dwork, nullptr);
  if (!rv && inflated) rv = f110qp_grid_inflate_dev(gc, dd2, radius, dout, nullptr);
  if (rv) {
    (void)hipStreamSynchronize(nullptr);
    return rv;
  }
  cp.back(d2, dd2, n * sizeof(int));
  cp.back(nearest, dnear, n * sizeof(int));
  cp.back(inflated, dout, n);
  const hipError_t es = hipStreamSynchronize(nullptr);  // the one synchronisation, also before `dev` is freed
  if (cp.e != hipSuccess) return hip_fail(cp.e, "field D2H");
  if (es != hipSuccess) return hip_fail(es, "field synchronise");
  return F110QP_OK;
}

int f110qp_wall_distance(const f110qp_grid_config* gc, const unsigned char* grid, int batch, int rows,
                         const double* x, double* dist, int* cell) {
  f110qp::GridParams Gr;
  if (const int rv = field_params(gc, grid, &Gr)) return rv;
  // the device call's rule on nearest and cell is this call's own business: it owns nearest
  if (const char* m = check_lookup(batch, rows, x, dist, cell, cell)) return fail(F110QP_ERR_INVALID, m);
  const size_t n = has_cells(Gr) ? (size_t)Gr.W * (size_t)Gr.H : 0, np = (size_t)rows * (size_t)batch;

  // one device buffer: the doubles (x, dist), the ints (cell, d2, nearest, work), the map
  DevBuf dev;
  hipError_t e = dev.ensure(4 * np * sizeof(double) + (np + 3 * n) * sizeof(int) + round8(n) + 8);
  if (e != hipSuccess) return hip_fail(e, "field staging allocation");
  double* dx = (double*)dev.p;
  double* ddist = dx + 3 * np;
  int* dcell = (int*)(ddist + np);
  int *dd2 = dcell + np, *dnear = dd2 + n, *dwork = dnear + n;
  unsigned char* dgrid = (unsigned char*)(dwork + n);
  Copies cp;
  cp.up(dgrid, grid, n);
  cp.up(dx, x, 3 * np * sizeof(double));
  if (cp.e != hipSuccess) {
    (void)hipStreamSynchronize(nullptr);
    return hip_fail(cp.e, "field H2D");
  }
  int rv = f110qp_grid_distance_dev(gc, n ? dgrid : nullptr, dd2, cell ? dnear : nullptr, dwork, nullptr);
  if (!rv)
    rv = f110qp_grid_lookup_dev(gc, n ? dd2 : nullptr, cell ? dnear : nullptr, batch, rows, dx, ddist,
                                cell ? dcell : nullptr, nullptr);
  if (rv) {
    (void)hipStreamSynchronize(nullptr);
    return rv;
  }
  cp.back(dist, ddist, np * sizeof(double));
  cp.back(cell, dcell, np * sizeof(int));
  const hipError_t es = hipStreamSynchronize(nullptr);  // the one synchronisation, also before `dev` is freed
  if (cp.e != hipSuccess) return hip_fail(cp.e, "field D2H");
  if (es != hipSuccess) return hip_fail(es, "field synchronise");
  return F110QP_OK;
}

}  // extern "C"
