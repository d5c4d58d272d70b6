// Host-only unit tests of the native runtime (CLI grammar, MT19937, report formats, stats, JSON,
// count parsing). Built twice: plainly (`make unit`) and under ASan+UBSan (`make asan`).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "mireduce/cli.hpp"
#include "mireduce/combo.hpp"
#include "mireduce/fault.hpp"
#include "mireduce/mt19937.hpp"
#include "mireduce/peer_access.hpp"
#include "mireduce/report.hpp"
#include "mireduce/timer.hpp"
#include "mireduce/types.hpp"

using namespace mireduce;

static int g_fail = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                           \
    }                                                                     \
  } while (0)

static void test_peer_plan() {
  // bandwidth_test --peer: ordered pairs, no self pairs, row-major; matrix table shape
  CHECK(peer_pairs(0).empty() && peer_pairs(1).empty());
  const auto p2 = peer_pairs(2);
  CHECK(p2.size() == 2 && p2[0] == std::make_pair(0, 1) && p2[1] == std::make_pair(1, 0));
  const auto p8 = peer_pairs(8);
  CHECK(p8.size() == 56);
  for (auto [s, d] : p8) CHECK(s != d && s >= 0 && d < 8);
  std::vector<double> v(9, 0.0);
  v[1] = 12.5;
  v[3] = 99.0;
  const std::string t = peer_matrix(3, v, "GB/s");
  CHECK(t.find("12.5") != std::string::npos && t.find("99.0") != std::string::npos);
  CHECK(t.find("(GB/s)") != std::string::npos);
  int lines = 0;
  for (char c : t) lines += c == '\n';
  CHECK(lines == 5);  // title, column header, 3 source rows
}

static void test_cli() {
  const char* argv[] = {"prog", "--method=SUM", "-type=double", "--cpufinal", "-n=16M", "--list=a,b,,c", "--neg=-5"};
  CmdArgs a(7, argv);
  std::string s;
  CHECK(a.program() == "prog");
  CHECK(a.get_str("method", &s) && s == "SUM");
  CHECK(a.get_str("type", &s) && s == "double");
  CHECK(a.has("cpufinal") && !a.get_str("cpufinal", &s));
  uint64_t n = 0;
  CHECK(a.get_uint("n", &n) && n == (16ull << 20));
  std::vector<std::string> l;
  CHECK(a.get_list("list", &l) && l.size() == 3 && l[2] == "c");
  int64_t v = 0;
  CHECK(a.get_int("neg", &v) && v == -5);
  CHECK(a.unknown({"method", "type", "cpufinal", "n", "list"}).size() == 1);
  bool threw = false;
  try {
    const char* bad[] = {"prog", "method=SUM"};
    CmdArgs b(2, bad);
  } catch (const CliError&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {
    const char* bad[] = {"prog", "--n=12x"};
    CmdArgs b(2, bad);
    uint64_t x;
    b.get_uint("n", &x);
  } catch (const CliError&) {
    threw = true;
  }
  CHECK(threw);
  uint64_t c = 0;
  CHECK(parse_count("1e9", &c) && c == 1000000000ull);
  CHECK(parse_count("4k", &c) && c == 4096);
  CHECK(parse_count("2G", &c) && c == (2ull << 30));
  CHECK(!parse_count("abc", &c) && !parse_count("1.5e0", &c));
}

static void test_types() {
  DType t;
  Op o;
  CHECK(parse_dtype("DOUBLE", &t) && t == DType::Float64);
  CHECK(parse_dtype("Int", &t) && t == DType::Int32);
  CHECK(parse_dtype("int64", &t) && t == DType::Int64);
  CHECK(!parse_dtype("char", &t));
  CHECK(parse_op_strict("SUM", &o) && o == Op::Sum);
  CHECK(!parse_op_strict("sum", &o));
  CHECK(parse_op("max", &o) && o == Op::Max);
  CHECK(default_acc(DType::Int32, Op::Sum) == DType::Int64);
  CHECK(default_acc(DType::Float32, Op::Min) == DType::Float32);
  CHECK(std::string(dtype_gnuplot_name(DType::Float64)) == "DOUBLE");
}

static void test_mt() {
  Mt19937 g;
  const uint64_t key[4] = {0x123, 0x234, 0x345, 0x456};
  g.init_by_array(key, 4);
  const uint32_t expect[5] = {1067595299u, 955945823u, 477289528u, 4107218783u, 4228976476u};
  for (uint32_t e : expect) CHECK(g.genrand_int32() == e);
  Mt19937 h(5489u);
  CHECK(h.genrand_int32() == 3499211612u);  // std::mt19937 default-seed first output
}

static void test_report() {
  CHECK(gnuplot_header() == "# DATATYPE OP NODES GB/sec");
  CHECK(gnuplot_line("INT", "SUM", 1024, 146.684) == "INT SUM 1024    146.684");
  CHECK(throughput_line(92.7729, 0.00072, 16777216, 1, 256) ==
        "Reduction, Throughput = 92.7729 GB/s, Time = 0.00072 s, Size = 16777216 Elements, NumDevsUsed = 1, Workgroup = 256");
  Stats s = compute_stats({3, 1, 2, 4});
  CHECK(s.count == 4 && s.min == 1 && s.max == 4 && s.median == 2.5 && std::fabs(s.mean - 2.5) < 1e-12);
  Json j;
  j.set("a", "x\"y").set("b", 1.5).set("c", static_cast<int64_t>(-3)).set("d", true).set("e", std::vector<double>{1, 2});
  CHECK(j.str() == "{\"a\": \"x\\\"y\", \"b\": 1.5, \"c\": -3, \"d\": true, \"e\": [1,2]}");
  StopWatch w;
  w.start();
  w.stop();
  w.start();
  w.stop();
  CHECK(w.sessions() == 2 && w.laps_ms().size() == 2 && w.average_ms() >= 0);
}

static void test_fault_spec() {
  FaultSpec f = parse_fault_spec("");
  CHECK(f.kind == FaultSpec::Kind::None);
  f = parse_fault_spec("exit");
  CHECK(f.kind == FaultSpec::Kind::Exit && f.rank == 1 && f.step == 0);
  f = parse_fault_spec("hang@3:17");
  CHECK(f.kind == FaultSpec::Kind::Hang && f.rank == 3 && f.step == 17);
  f = parse_fault_spec("delay=250@0:2");
  CHECK(f.kind == FaultSpec::Kind::Delay && f.delay_ms == 250 && f.rank == 0 && f.step == 2);
  f = parse_fault_spec("corrupt:5");
  CHECK(f.kind == FaultSpec::Kind::Corrupt && f.rank == 1 && f.step == 5);
  for (const char* bad : {"boom", "exit@", "exit@x", "hang:-1", "delay=", "corrupt@1:2x"}) {
    bool threw = false;
    try {
      parse_fault_spec(bad);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    CHECK(threw);
  }
  FaultInjector inj(parse_fault_spec("corrupt@2:4"));
  CHECK(!inj.at(1, 4, "unit") && !inj.at(2, 3, "unit"));
  CHECK(inj.at(2, 4, "unit"));
  CHECK(!inj.at(2, 4, "unit"));  // fires once
  FaultInjector d(parse_fault_spec("delay=1@0:0"));
  CHECK(!d.at(0, 0, "unit"));
}

static void test_peer_verdict() {
  // the native twin of parallel/topology.py peer_verdict
  auto yes = [](int, int) { return true; };
  auto no = [](int, int) { return false; };
  const std::vector<PeerKey> node = {{"h", "g0", 0}, {"h", "g1", 1}, {"h", "g2", 2}};
  for (int me = 0; me < 3; ++me) CHECK(peer_verdict(node, me, yes).empty());
  CHECK(peer_verdict(node, 1, no) == "device 1 cannot access peer device 0 (rank 0)");
  // a one-way link: 0 can map 2 but 2 cannot map 0 -> only rank 2 objects
  auto oneway = [](int a, int b) { return !(a == 2 && b == 0); };
  CHECK(peer_verdict(node, 0, oneway).empty());
  CHECK(peer_verdict(node, 2, oneway).find("cannot access peer device 0") != std::string::npos);
  // ranks sharing one physical GPU need no peer access (one-GPU rehearsals)
  const std::vector<PeerKey> shared = {{"h", "g0", 0}, {"h", "g0", 0}, {"h", "g0", 0}};
  CHECK(peer_verdict(shared, 2, no).empty());
  // another host: IPC handles do not cross hosts
  const std::vector<PeerKey> two_hosts = {{"a", "g0", 0}, {"b", "g0", 0}};
  CHECK(peer_verdict(two_hosts, 0, yes).find("runs on host b") != std::string::npos);
  // same index, different GPU (e.g. different visibility masks)
  const std::vector<PeerKey> alias = {{"h", "g0", 0}, {"h", "g7", 0}};
  CHECK(peer_verdict(alias, 1, yes).find("a different GPU") != std::string::npos);
  CHECK(peer_verdict(node, 5, yes) == "rank index out of range");
  // agreement: identical text on every rank, failing ranks only, in rank order
  CHECK(agree_verdicts({"", "", ""}).empty());
  CHECK(agree_verdicts({"", "x", "", "y"}) == "rank 1: x; rank 3: y");
  // the injected fault kind parses and is not a step fault
  FaultInjector f(parse_fault_spec("nopeer@1"));
  CHECK(f.no_peer(1) && !f.no_peer(0) && !f.at(1, 0, "unit"));
}

// combo.hpp's list against types.hpp's predicates, and the numbering that tuning JSON and the
// flat kernel's dispatch table are keyed by.
static int combo_index_before_the_list(Op op, DType t, DType acc) {
  constexpr DType I32 = DType::Int32, I64 = DType::Int64, F32 = DType::Float32, F64 = DType::Float64,
                  BF16 = DType::BFloat16, F16 = DType::Float16;
  static const struct { Op op; DType t, acc; } numbered[29] = {
      {Op::Sum, I32, I64},      {Op::Sum, I32, I32},     {Op::Min, I32, I32},      {Op::Max, I32, I32},      // 0..3
      {Op::Sum, I64, I64},      {Op::Min, I64, I64},     {Op::Max, I64, I64},                                // 4..6
      {Op::Sum, F32, F64},      {Op::Sum, F32, F32},     {Op::Min, F32, F32},      {Op::Max, F32, F32},      // 7..10
      {Op::Sum, F64, F64},      {Op::Min, F64, F64},     {Op::Max, F64, F64},                                // 11..13
      {Op::Sum, BF16, F32},     {Op::Min, BF16, F32},    {Op::Max, BF16, F32},                               // 14..16
      {Op::Sum, F16, F32},      {Op::Min, F16, F32},     {Op::Max, F16, F32},                                // 17..19
      {Op::SumSq, F32, F64},    {Op::SumSq, F32, F32},   {Op::SumSq, F64, F64},                              // 20..22
      {Op::SumSq, BF16, F32},   {Op::SumSq, F16, F32},                                                       // 23..24
      {Op::AbsMax, F32, F32},   {Op::AbsMax, F64, F64},  {Op::AbsMax, BF16, F32},  {Op::AbsMax, F16, F32}};  // 25..28
  for (int i = 0; i < 29; ++i)
    if (numbered[i].op == op && numbered[i].t == t && numbered[i].acc == acc) return i;
  return -1;
}

static void test_combos() {
  const Op ops[] = {Op::Sum, Op::Min, Op::Max, Op::SumSq, Op::AbsMax};
  const DType types[] = {DType::Int32, DType::Int64, DType::Float32, DType::Float64, DType::BFloat16, DType::Float16};
  CHECK(kCombos == 29);
  int supported = 0;
  bool seen[kCombos] = {};
  for (DType t : types)
    for (Op op : ops) {
      bool any = false;
      for (DType acc : types) {
        int visits = 0;
        const bool found = visit_combo(op, t, acc, [&](auto c) {
          using C = decltype(c);
          ++visits;
          CHECK(sizeof(typename C::elem) == dtype_size(t) && dtype_of<typename C::elem>::value == t);
          CHECK(sizeof(typename C::acc) == dtype_size(acc) && dtype_of<typename C::acc>::value == acc);
          CHECK(op_of<typename C::op>::value == op);
          CHECK((std::is_same_v<typename C::op, SumOp>) == (op == Op::Sum));
          CHECK((std::is_same_v<typename C::op, MinOp>) == (op == Op::Min));
          CHECK((std::is_same_v<typename C::op, MaxOp>) == (op == Op::Max));
          CHECK((std::is_same_v<typename C::op, SumSqOp>) == (op == Op::SumSq));
          CHECK((std::is_same_v<typename C::op, AbsMaxOp>) == (op == Op::AbsMax));
        });
        CHECK(found == acc_supported(t, op, acc));
        CHECK(visits == (found ? 1 : 0));
        const int i = combo_index(op, t, acc);
        CHECK(i == combo_index_before_the_list(op, t, acc));
        CHECK(found == (i >= 0));
        if (i >= 0 && i < kCombos) {
          CHECK(!seen[i]);
          seen[i] = true;
        }
        supported += found ? 1 : 0;
        any = any || found;
        // the operator subset: the fused operators are not found, the others as before
        const bool plain = visit_combo<PlainOps>(op, t, acc, [](auto) {});
        CHECK(plain == (found && !op_is_fused(op)));
      }
      if (any) CHECK(combo_index(op, t, default_acc(t, op)) >= 0);
    }
  CHECK(supported == 29);
  for (bool s : seen) CHECK(s);
  int visited = 0;
  CHECK(visit_dtype(DType::BFloat16, [&](auto z) { visited += std::is_same_v<decltype(z), bf16_t> ? 1 : 0; }));
  CHECK(visited == 1 && !visit_dtype(static_cast<DType>(99), [](auto) {}));
}

int main() {
  test_combos();
  test_peer_verdict();
  test_cli();
  test_peer_plan();
  test_fault_spec();
  test_types();
  test_mt();
  test_report();
  if (g_fail) {
    std::fprintf(stderr, "host_unit: %d failures\n", g_fail);
    return 1;
  }
  std::printf("host_unit: all checks passed\n");
  return 0;
}
