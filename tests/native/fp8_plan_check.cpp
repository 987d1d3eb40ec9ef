// What the host-side kernel API says about the two OCP FP8 dtypes (tests/test_fp8_cpu.py): element
// size, supported ops, and that kern::ipc_plan treats an FP8 reduction exactly like the int8 one of
// the same bytes (same rejection, grid and kernel family) while keeping the FP8 dtype. Host only:
// no GPU, no HIP runtime call. Built with ASan + UBSan. Exit status 0 and "ok <checks>" on success.
#include <cstdio>

#include "kernels/ipc_plan.h"

using namespace pdcc::kern;

static int g_checks = 0, g_bad = 0;
#define CHECK(cond, ...)            \
  do {                              \
    ++g_checks;                     \
    if (!(cond)) {                  \
      ++g_bad;                      \
      printf("FAIL: " __VA_ARGS__); \
      printf("\n");                 \
    }                               \
  } while (0)

static IpcCall call(IpcColl coll, DType dt, RedOp op, int world, size_t bytes, int zc) {
  IpcCall c{};
  c.coll = coll;
  c.dtype = dt;
  c.op = op;
  c.root = world - 1;
  c.avg_div = world;
  c.zc = zc;
  c.bytes = bytes;
  return c;
}

int main() {
  // the first nine values and their count are what the recorded plan golden was taken over
  CHECK((int)DType::kCount == 9, "kCount = %d", (int)DType::kCount);
  CHECK((int)DType::F8E4M3 == 9 && (int)DType::F8E5M2 == 10 && (int)DType::kEnd == 11, "FP8 values moved");
  for (DType dt : {DType::F8E4M3, DType::F8E5M2}) {
    const int d = (int)dt;
    CHECK(dtype_size(dt) == 1, "dtype_size(%d) = %zu", d, dtype_size(dt));
    for (RedOp op : {RedOp::SUM, RedOp::AVG, RedOp::PROD, RedOp::MIN, RedOp::MAX, RedOp::COPY})
      CHECK(supports(dt, op), "supports(%d, %d) is false", d, (int)op);
    for (RedOp op : {RedOp::BAND, RedOp::BOR, RedOp::BXOR})
      CHECK(!supports(dt, op), "supports(%d, %d) is true", d, (int)op);
    for (int coll = 0; coll < (int)IpcColl::kCount; ++coll) {
      if (!coll_traits((IpcColl)coll).reducing) continue;
      for (int w : {2, 3, 8})
        for (size_t bytes : {(size_t)1, (size_t)4096, (size_t)262144, (size_t)3 * 4096 * w})
          for (int zc = 0; zc < 2; ++zc)
            for (RedOp op : {RedOp::SUM, RedOp::MAX}) {
              const IpcCall f = call((IpcColl)coll, dt, op, w, bytes, zc);
              const IpcCall i = call((IpcColl)coll, DType::I8, op, w, bytes, zc);
              const IpcPlan pf = ipc_plan(w, f), pi = ipc_plan(w, i);
              CHECK(pf.err == pi.err && pf.grid == pi.grid && pf.family == pi.family,
                    "coll %d w %d bytes %zu zc %d op %d: fp8 err %d grid %d family %d, int8 err %d grid %d family %d",
                    coll, w, bytes, zc, (int)op, (int)pf.err, pf.grid, (int)pf.family, (int)pi.err, pi.grid,
                    (int)pi.family);
              CHECK(pf.dtype == dt && pf.op == op, "coll %d w %d bytes %zu: plan dtype %d op %d", coll, w, bytes,
                    (int)pf.dtype, (int)pf.op);
              CHECK(ipc_staging_bytes(f, w) == ipc_staging_bytes(i, w), "coll %d w %d bytes %zu zc %d: staging", coll,
                    w, bytes, zc);
            }
      // bitwise ops: rejected for FP8, accepted for int8
      const IpcPlan pb = ipc_plan(2, call((IpcColl)coll, dt, RedOp::BXOR, 2, 4096, 0));
      CHECK(pb.err != hipSuccess, "coll %d: BXOR on dtype %d accepted", coll, d);
    }
  }
  printf("%s %d\n", g_bad ? "failed" : "ok", g_checks);
  return g_bad ? 1 : 0;
}
