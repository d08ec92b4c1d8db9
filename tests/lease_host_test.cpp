// Stand-alone host test of nsk::Lease and nsk::SlotLease (nsk_core.hpp): no device is touched — the pool's free list is
// filled with host memory, and VecPool::get(false) on a non-empty free list makes no HIP call.
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "nsk_core.hpp"

using namespace nsk;

static int failures = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } \
  } while (0)

static void thrower(VecPool &pool, Ctx &ctx) {
  Lease a(pool, false), b(pool, false);
  SlotLease s(ctx, 3);
  CHECK(pool.free_list.size() == 2 && ctx.slot_top == 3);
  throw Error(-1, "on purpose");
}

int main() {
  static_assert(!std::is_copy_constructible<Lease>::value && !std::is_copy_assignable<Lease>::value, "Lease is move-only");
  static_assert(!std::is_copy_constructible<SlotLease>::value, "SlotLease does not copy");
  std::vector<std::vector<double>> mem(4, std::vector<double>(8, 0.0));
  Ctx ctx;
  VecPool pool;
  pool.init(&ctx, 8, 0);
  for (auto &m : mem) pool.put(m.data());
  {
    Lease a(pool, false);
    CHECK(pool.free_list.size() == 3 && (double *)a == mem[3].data());   // LIFO
    a[0] = 1.0;                                                          // converts to double *
    Lease b(std::move(a));                                               // move construction: one owner
    CHECK((double *)a == nullptr && (double *)b == mem[3].data() && pool.free_list.size() == 3);
    Lease c(pool, false);
    c = std::move(b);                                                    // move assignment: c's old vector goes back first
    CHECK(pool.free_list.size() == 3 && pool.free_list.back() == mem[2].data() && (double *)c == mem[3].data());
    c.release();
    c.release();                                                         // a second release does nothing
    CHECK(pool.free_list.size() == 4 && pool.free_list.back() == mem[3].data());
  }
  CHECK(pool.free_list.size() == 4);                                     // nothing went back twice
  {
    double *v = pool.get(false);
    const Lease l = Lease::adopt(pool, v);
    CHECK(pool.free_list.size() == 3);
  }
  CHECK(pool.free_list.size() == 4);
  bool caught = false;
  try {
    thrower(pool, ctx);
  } catch (const Error &) {
    caught = true;
  }
  CHECK(caught && pool.free_list.size() == 4 && ctx.slot_top == 0);      // release on throw
  {
    SlotLease s(ctx, 2);
    const int later = ctx.alloc_slots(5);                                // slots taken after the lease go with it
    CHECK((int)s == 0 && later == 2 && ctx.slot_top == 7);
  }
  CHECK(ctx.slot_top == 0);
  std::vector<Lease> held;                                               // leases in a container (nsk_time_op)
  for (int k = 0; k < 3; ++k) held.emplace_back(pool, false);
  CHECK(pool.free_list.size() == 1);
  held.clear();
  CHECK(pool.free_list.size() == 4);
  std::printf(failures ? "lease host test: %d failure(s)\n" : "lease host test: ok\n", failures);
  return failures ? 1 : 0;
}
