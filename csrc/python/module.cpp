// pybind11 bindings: the native miint runtime + kernels as `cuda_v_mpi_amd._miint`.
//
// Device memory crosses the boundary as integer addresses (torch.Tensor.data_ptr()) and
// streams as integer handles (torch.cuda.Stream.cuda_stream), so the module has no libtorch
// ABI dependency and no hipify step; it links only libamdhip64 and librccl.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "miint/comm.hpp"
#include "miint/expr.hpp"
#include "miint/fast_trig.hpp"
#include "miint/host.hpp"
#include "miint/integrator.hpp"
#include "miint/kernels.hpp"
#include "miint/oracle.hpp"
#include "miint/runtime.hpp"
#include "miint/selftest.hpp"
#include "miint/table2d.hpp"
#include "miint/trace.hpp"
#include "miint/trainscan.hpp"

namespace py = pybind11;
using namespace miint;

namespace {

template <typename T>
T* ptr(uintptr_t p) { return reinterpret_cast<T*>(p); }
hipStream_t stream(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

RiemannParams make_params(int integrand, double a, double h, double off, uint64_t i_begin,
                          uint64_t n, const std::vector<double>& coef, double p0, double p1,
                          const std::string& tile = "auto") {
  RiemannParams p{};
  p.a = a;
  p.h = h;
  p.off = off;
  p.i_begin = i_begin;
  p.n = n;
  p.integrand = integrand;
  MIINT_CHECK(coef.size() <= static_cast<size_t>(kMaxPolyCoeffs), "too many coefficients");
  p.ncoef = static_cast<int>(coef.size());
  for (size_t i = 0; i < coef.size(); ++i) p.coef[i] = coef[i];
  p.p0 = p0;
  p.p1 = p1;
  p.tile = tile_form_of(tile);
  return p;
}

// Sweep parameters: a list of rows or a 2-D float64 array, K x nparams -> row-major values.
// An empty sequence is K = 0; ragged or non-numeric rows are refused here.
using ParamRows = py::object;
std::vector<double> param_rows(const ParamRows& obj, int nparams, uint64_t* rows) {
  auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(obj);
  if (!arr) {
    PyErr_Clear();
    fail("expression sweep: params must be K rows of " + std::to_string(nparams) +
             " numbers (a list of rows or a 2-D float64 array)", __FILE__, __LINE__);
  }
  if (arr.size() == 0 && arr.ndim() >= 1 && arr.shape(0) == 0) {
    *rows = 0;
    return {};
  }
  MIINT_CHECK(arr.ndim() == 2, "expression sweep: params must be 2-D (K rows x nparams)");
  MIINT_CHECK(arr.shape(1) == nparams,
              "expression sweep: rows of " + std::to_string(arr.shape(1)) +
                  " values, the expression was built for nparams = " + std::to_string(nparams));
  *rows = static_cast<uint64_t>(arr.shape(0));
  return std::vector<double>(arr.data(), arr.data() + arr.size());
}

// A binding of a hipRTC compile (expr_compile and its kin): the GIL released, the code object
// as bytes.
template <class... A>
auto compiled(std::string (*compile)(A...)) {
  return [compile](A... a) {
    std::string code;
    {
      py::gil_scoped_release nogil;
      code = compile(a...);
    }
    return py::bytes(code);
  };
}

}  // namespace

static const char* scan_algo_name(ScanAlgo a) {
  return a == ScanAlgo::kFused ? "fused" : a == ScanAlgo::kOnePass ? "onepass" : "lookback";
}
static ScanAlgo scan_algo_of(const std::string& s) {
  MIINT_CHECK(s == "fused" || s == "lookback" || s == "onepass",
              "algo must be onepass|fused|lookback");
  return s == "fused" ? ScanAlgo::kFused : s == "onepass" ? ScanAlgo::kOnePass : ScanAlgo::kLookback;
}

PYBIND11_MODULE(_miint, m) {
  m.doc() = "miint: MI355X-native numerical integration (HIP/gfx950 kernels, RCCL, hipGraph)";
  py::register_exception<miint::Error>(m, "MiintError", PyExc_RuntimeError);
  install_crash_handler_from_env();

  // ------------------------------------------------------------------ enums
  py::enum_<Integrand>(m, "Integrand")
      .value("pi4", Integrand::kPi4)
      .value("sin", Integrand::kSin)
      .value("poly", Integrand::kPoly)
      .value("train", Integrand::kTrainVel)
      .value("table", Integrand::kTable);
  py::enum_<Rule>(m, "Rule").value("left", Rule::kLeft).value("mid", Rule::kMid).value("right", Rule::kRight);
  py::enum_<DType>(m, "DType")
      .value("fp64", DType::kF64)
      .value("fp32", DType::kF32)
      .value("fp32acc", DType::kF32Acc32);
  py::enum_<DivMode>(m, "DivMode")
      .value("series", DivMode::kSeries)
      .value("ieee", DivMode::kIeee)
      .value("series_direct", DivMode::kSeriesDirect)
      .value("series_exact", DivMode::kSeriesExact);

  m.attr("TICKET_WORDS") = kTicketWords;
  m.attr("UNSET_SLOT_WORD") = kUnsetSlotWord;
  m.def("fill_unset_slots", [](uintptr_t p, size_t count, uintptr_t s) {
    fill_unset_slots(ptr<double>(p), count, stream(s));
  });
  m.attr("RIEMANN_TILE") = kRiemannTile;
  m.attr("RIEMANN_BLOCK") = kRiemannBlock;
  m.def("series_ok", &series_ok);
  m.def("series_ok_f32", &series_ok_f32);
  m.def("integrand_scale", &integrand_scale);

  // ------------------------------------------------------------------ devices
  m.def("device_count", &device_count);
  m.def("device_info", [](int d) {
    DeviceInfo i = device_info(d);
    py::dict r;
    r["index"] = i.index;
    r["name"] = i.name;
    r["arch"] = i.arch;
    r["num_cus"] = i.num_cus;
    r["clock_khz"] = i.clock_khz;
    r["total_mem"] = i.total_mem;
    r["l2_bytes"] = i.l2_bytes;
    return r;
  });
  m.def("set_device", &set_device);
  m.def("device_synchronize", []() { MIINT_HIP(hipDeviceSynchronize()); });
  // Host wait policy of the current device (hipDeviceSchedule*): "spin" polls the completion
  // signal (lowest wake-up latency, one busy core per waiting thread), "yield", "blocking"
  // (interrupt), "auto" (the runtime's default).
  m.def("set_device_flags", [](const std::string& mode) {
    unsigned f = hipDeviceScheduleAuto;
    if (mode == "spin") f = hipDeviceScheduleSpin;
    else if (mode == "yield") f = hipDeviceScheduleYield;
    else if (mode == "blocking") f = hipDeviceScheduleBlockingSync;
    else if (mode != "auto") throw std::invalid_argument("spin|yield|blocking|auto");
    MIINT_HIP(hipSetDeviceFlags(f));
  });
  m.def("get_device_flags", []() {
    unsigned f = 0;
    MIINT_HIP(hipGetDeviceFlags(&f));
    return f;
  });
  m.def("process_start_seconds", &process_start_seconds);
  m.def("enable_tracing", &enable_tracing, py::arg("on"),
        "roctx ranges around runtime phases (MIINT_ROCTX=1)");
  m.def("tracing_enabled", &tracing_enabled);
  m.def("trace_mark", &trace_mark);
  m.def("wait_with_timeout", [](uintptr_t s, double timeout_s) {
    py::gil_scoped_release nogil;
    return wait_with_timeout(stream(s), timeout_s, nullptr);
  });
  m.def("wall_seconds", &wall_seconds);

  // ------------------------------------------------------------------ comm
  py::class_<Comm>(m, "Communicator")
      .def_property_readonly("rank", &Comm::rank)
      .def_property_readonly("world", &Comm::world)
      .def_property_readonly("device", &Comm::device)
      .def_property_readonly("kind", [](const Comm& c) { return std::string(c.kind()); })
      .def_property_readonly("transport_world", &Comm::transport_world,
                             "ranks the transport reports (ncclCommCount for RCCL)")
      .def("allreduce_sum", [](const Comm& c, uintptr_t send, uintptr_t recv, size_t count,
                               uintptr_t s) {
             py::gil_scoped_release nogil;  // loopback collectives barrier across threads
             c.allreduce_sum(ptr<double>(send), ptr<double>(recv), count, stream(s));
           })
      .def("allgather", [](const Comm& c, uintptr_t send, uintptr_t recv, size_t count,
                           uintptr_t s) {
             py::gil_scoped_release nogil;
             c.allgather(ptr<double>(send), ptr<double>(recv), count, stream(s));
           })
      .def("broadcast", [](const Comm& c, uintptr_t buf, size_t count, int root, uintptr_t s) {
        py::gil_scoped_release nogil;
        c.broadcast(ptr<double>(buf), count, root, stream(s));
      })
      .def("reduce_sum", [](const Comm& c, uintptr_t send, uintptr_t recv, size_t count,
                            int root, uintptr_t s) {
        py::gil_scoped_release nogil;
        c.reduce_sum(ptr<double>(send), ptr<double>(recv), count, root, stream(s));
      })
      .def("check_async", &Comm::check_async);
  py::class_<RcclComm, Comm>(m, "Comm")
      .def(py::init([](py::bytes id, int rank, int world, int device) {
             return new RcclComm(std::string(id), rank, world, device);
           }),
           py::arg("unique_id"), py::arg("rank"), py::arg("world"), py::arg("device"))
      .def_static("unique_id", []() { return py::bytes(RcclComm::unique_id()); })
      .def_static("version", &RcclComm::version);
  py::class_<LoopbackComm, Comm>(m, "LoopbackComm");
  py::class_<LoopbackGroup, std::shared_ptr<LoopbackGroup>>(m, "LoopbackGroup",
      "W logical ranks on one device (test transport; drive rank r from its own thread)")
      .def(py::init(&LoopbackGroup::create), py::arg("world"), py::arg("device") = 0,
           py::arg("timeout_s") = 120.0)
      .def_property_readonly("world", &LoopbackGroup::world)
      .def_property_readonly("device", &LoopbackGroup::device)
      .def("comm", &LoopbackGroup::comm, py::arg("rank"), py::return_value_policy::reference_internal)
      .def("barrier", &LoopbackGroup::barrier, py::arg("rank"), py::call_guard<py::gil_scoped_release>())
      .def("mark_broken", &LoopbackGroup::mark_broken)
      .def_property_readonly("broken", &LoopbackGroup::broken)
      .def_property_readonly("collectives", &LoopbackGroup::collectives)
      .def_property_readonly("graph_launches", &LoopbackGroup::graph_launches);
  m.def(
      "rendezvous_unique_id",
      [](const std::string& addr, int port, int rank, int world, double timeout_s) {
        std::string id;
        {
          py::gil_scoped_release rel;  // rank 0 blocks in accept() until the others connect
          id = rendezvous_unique_id(addr, port, rank, world, timeout_s);
        }
        return py::bytes(id);  // 128 raw bytes, not text
      },
      py::arg("addr"), py::arg("port"), py::arg("rank"), py::arg("world"),
      py::arg("timeout_s") = 120.0);
  // RCCL transport evidence (miint/comm.hpp): which transport the ranks' connections use
  auto transport_dict = [](const RcclTransport& t) {
    py::dict d;
    d["transport"] = t.transport;
    d["nranks"] = t.nranks;
    d["nnodes"] = t.nnodes;
    d["local_ranks"] = t.local_ranks;
    d["connections"] = t.connections;
    d["comms"] = t.comms;
    d["uses_net"] = t.uses_net();
    d["log"] = t.log;
    return d;
  };
  m.def("parse_rccl_log", [transport_dict](const std::string& text) {
    return transport_dict(parse_rccl_log(text));
  });
  m.def("capture_rccl_log", &capture_rccl_log,
        "route RCCL's INIT log into a per-process file (call before the first RCCL call)");
  m.def("rccl_log_path", &rccl_log_path);
  m.def("rccl_transport", [transport_dict]() { return transport_dict(rccl_transport()); });
  m.def(
      "transport_error",
      [](const std::string& log_text, int world, int local_world, bool share) {
        return transport_error(parse_rccl_log(log_text), world, local_world, share);
      },
      "the native CLIs' fail-closed transport verdict on an RCCL INIT log (\"\" = ok)",
      py::arg("log_text"), py::arg("world"), py::arg("local_world"), py::arg("share"));

  // ------------------------------------------------------------------ Riemann plan
  py::class_<RiemannConfig>(m, "RiemannConfig")
      .def(py::init<>())
      .def_readwrite("integrand", &RiemannConfig::integrand)
      .def_readwrite("a", &RiemannConfig::a)
      .def_readwrite("b", &RiemannConfig::b)
      .def_readwrite("n", &RiemannConfig::n)
      .def_readwrite("rule", &RiemannConfig::rule)
      .def_readwrite("dtype", &RiemannConfig::dtype)
      .def_readwrite("div", &RiemannConfig::div)
      .def_readwrite("coef", &RiemannConfig::coef)
      .def_readwrite("p0", &RiemannConfig::p0)
      .def_readwrite("p1", &RiemannConfig::p1)
      .def_readwrite("table", &RiemannConfig::table)
      .def_readwrite("grid", &RiemannConfig::grid)
      .def_readwrite("block", &RiemannConfig::block)
      .def_readwrite("waves_per_cu", &RiemannConfig::waves_per_cu)
      .def_readwrite("fused", &RiemannConfig::fused)
      .def_readwrite("slots", &RiemannConfig::slots)
      .def_readwrite("bucket", &RiemannConfig::bucket)
      .def_readwrite("rank", &RiemannConfig::rank)
      .def_readwrite("world", &RiemannConfig::world)
      .def_readwrite("force_collective", &RiemannConfig::force_collective)
      .def_readwrite("step_streams", &RiemannConfig::step_streams)
      .def_readwrite("multistep", &RiemannConfig::multistep)
      .def_readwrite("slice_rank", &RiemannConfig::slice_rank)
      .def_readwrite("slice_world", &RiemannConfig::slice_world)
      .def_readwrite("timeout_s", &RiemannConfig::timeout_s)
      .def_readwrite("host_direct", &RiemannConfig::host_direct)
      .def_readwrite("close", &RiemannConfig::close)
      .def_readwrite("work", &RiemannConfig::work)
      .def_readwrite("tile", &RiemannConfig::tile)
      .def_readwrite("queue_wg_per_cu", &RiemannConfig::queue_wg_per_cu)
      .def_readwrite("allreduce_to_host", &RiemannConfig::allreduce_to_host)
      .def_readwrite("chain", &RiemannConfig::chain);

  py::class_<RiemannPlan>(m, "RiemannPlan")
      .def(py::init<const RiemannConfig&, int, const Comm*>(), py::arg("config"),
           py::arg("device"), py::arg("comm") = nullptr, py::keep_alive<1, 4>())
      .def_property_readonly("device", &RiemannPlan::device)
      .def_property_readonly("rank", &RiemannPlan::rank)
      .def_property_readonly("world", &RiemannPlan::world)
      .def("step_streams", &RiemannPlan::step_streams, py::arg("nsteps"))
      .def_property_readonly("begin", &RiemannPlan::begin)
      .def_property_readonly("count", &RiemannPlan::count)
      .def_property_readonly("h", &RiemannPlan::h)
      .def_property_readonly("scale", &RiemannPlan::scale)
      .def_property_readonly("grid", [](const RiemannPlan& p) { return p.shape().grid; })
      .def_property_readonly("block", [](const RiemannPlan& p) { return p.shape().block; })
      .def_property_readonly("effective_div", &RiemannPlan::effective_div)
      .def_property_readonly("compute_stream", [](const RiemannPlan& p) { return reinterpret_cast<uintptr_t>(p.compute_stream()); })
      .def_property_readonly("comm_stream", [](const RiemannPlan& p) { return reinterpret_cast<uintptr_t>(p.comm_stream()); })
      .def("run", &RiemannPlan::run, py::call_guard<py::gil_scoped_release>())
      .def("capture_graphs", &RiemannPlan::capture_graphs, py::call_guard<py::gil_scoped_release>())
      .def("prepare_steps", &RiemannPlan::prepare_steps, py::arg("steps"),
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("graph_launches", &RiemannPlan::graph_launches)
      .def_property_readonly("direct_steps", &RiemannPlan::direct_steps)
      .def("launch_steps", &RiemannPlan::launch_steps, py::arg("steps"), py::arg("pipeline") = true,
           py::arg("graphs") = true, py::call_guard<py::gil_scoped_release>())
      .def("sync", &RiemannPlan::sync, py::call_guard<py::gil_scoped_release>())
      .def("run_steps", [](RiemannPlan& p, int steps, bool pipeline, bool graphs) {
             StepTiming t;
             {
               py::gil_scoped_release nogil;
               t = p.run_steps(steps, pipeline, graphs);
             }
             py::dict r;
             r["wall_s"] = t.wall_s;
             r["device_ms"] = t.device_ms;
             r["steps"] = t.steps;
             return r;
           }, py::arg("steps"), py::arg("pipeline") = true, py::arg("graphs") = true)
      .def("barrier", &RiemannPlan::barrier, py::call_guard<py::gil_scoped_release>())
      .def("time_one_shot", [](RiemannPlan& p, int reps, const std::string& mode, int warmup) {
             OneShotTiming t;
             {
               py::gil_scoped_release nogil;
               t = p.time_one_shot(reps, mode, warmup);
             }
             py::dict r;
             r["mode"] = t.mode;
             r["reps"] = t.reps;
             r["median_us"] = t.median_us;
             r["min_us"] = t.min_us;
             r["max_us"] = t.max_us;
             r["device_median_us"] = t.device_median_us;
             r["device_min_us"] = t.device_min_us;
             r["value"] = t.value;
             return r;
           }, py::arg("reps"), py::arg("mode") = "direct", py::arg("warmup") = 400)
      .def("diagnose_batch", [](RiemannPlan& p, int steps) {
             BatchDiag d;
             {
               py::gil_scoped_release nogil;
               d = p.diagnose_batch(steps);
             }
             py::dict r;
             r["steps"] = d.steps;
             r["compute_us"] = d.compute_us;
             r["close_us"] = d.close_us;
             r["allreduce_us"] = d.allreduce_us;
             r["copy_us"] = d.copy_us;
             r["tail_us"] = d.tail_us();
             r["boundary_us"] = d.boundary_us();
             r["marker_us"] = d.marker_us;
             r["device_us"] = d.device_us;
             r["staged_us"] = d.staged_us;
             r["wall_us"] = d.wall_us;
             return r;
           }, py::arg("steps"))
      .def("timeline_batch", [](RiemannPlan& p, int steps, const std::string& form) {
             BatchTimeline t;
             {
               py::gil_scoped_release nogil;
               t = p.timeline_batch(steps, form);
             }
             // numpy arrays (copies): stamps [grid, steps + 2], shader_clock and hw [grid, 2]
             auto arr64 = [](const std::vector<uint64_t>& v, py::ssize_t rows, py::ssize_t cols) {
               py::array_t<uint64_t> a({rows, cols});
               std::copy(v.begin(), v.end(), a.mutable_data());
               return a;
             };
             // a queue plan's record is per physical workgroup and per item (BatchTimeline)
             const bool queue = t.work == "queue";
             const py::ssize_t rows = queue ? t.workgroups : t.grid;
             py::array_t<uint32_t> hw({rows, py::ssize_t(2)});
             std::copy(t.hw.begin(), t.hw.end(), hw.mutable_data());
             py::dict r;
             r["steps"] = t.steps;
             r["grid"] = t.grid;
             r["block"] = t.block;
             r["clock_khz"] = t.clock_khz;
             r["device_us"] = t.device_us;
             r["work"] = t.work;
             if (queue) {
               r["workgroups"] = t.workgroups;
               r["wg_stamps"] = arr64(t.wg_stamps, rows, 2);
               r["item_stamp"] = arr64(t.item_stamp, t.steps, t.grid);
               py::array_t<uint32_t> owner({static_cast<py::ssize_t>(t.steps),
                                            static_cast<py::ssize_t>(t.grid)});
               std::copy(t.item_owner.begin(), t.item_owner.end(), owner.mutable_data());
               r["item_owner"] = owner;
             } else {
               r["stamps"] = arr64(t.stamps, t.grid, t.steps + 2);
             }
             r["shader_clock"] = arr64(t.shader_clock, rows, 2);
             r["hw"] = hw;
             r["values"] = t.values;
             return r;
           }, py::arg("steps"), py::arg("form") = "auto")
      .def("host_result", &RiemannPlan::host_result)
      .def_property_readonly("host_capacity", &RiemannPlan::host_capacity)
      .def_property_readonly("slots", &RiemannPlan::slots)
      .def_property_readonly("bucketed", &RiemannPlan::bucketed)
      .def_property_readonly("chained", &RiemannPlan::chained)
      .def_property_readonly("multistep", &RiemannPlan::multistep)
      .def_property_readonly("close_in_launch", &RiemannPlan::close_in_launch)
      .def_property_readonly("work", [](const RiemannPlan& p) { return std::string(p.work()); })
      .def_property_readonly("tile", [](const RiemannPlan& p) { return std::string(p.tile()); })
      .def_property_readonly("queue_workgroups", &RiemannPlan::queue_workgroups)
      .def_property_readonly("allreduce_to_host", &RiemannPlan::allreduce_to_host)
      .def_property_readonly("direct", &RiemannPlan::direct)
      .def_property_readonly("graph_nodes", &RiemannPlan::graph_nodes)
      .def_property_readonly("graphs_ready", &RiemannPlan::graphs_ready)
      .def_property_readonly("graph_error", &RiemannPlan::graph_error)
      .def_property_readonly("collective", &RiemannPlan::collective)
      .def("host_index_of", &RiemannPlan::host_index_of, py::arg("k"), py::arg("graphs"))
      .def("enqueue", [](const RiemannPlan& p, uintptr_t s, int slot, int hidx) { p.enqueue(stream(s), slot, hidx); })
      .def("device_result", [](const RiemannPlan& p, int slot) { return reinterpret_cast<uintptr_t>(p.device_result(slot)); });

  // ------------------------------------------------------------------ raw kernels
  // (each raw launcher also takes a trailing `tile`: "auto" | "short" | "long", the tile form
  // of the fp64 series_exact pi4 kernels, RiemannParams::tile)
  auto partials_fn = [](int integrand, double a, double h, double off, uint64_t i_begin,
                        uint64_t n, std::vector<double> coef, double p0, double p1, DType dtype,
                        DivMode div, int grid, uintptr_t table, int table_n, uintptr_t partials,
                        uintptr_t s, const std::string& tile) {
    const RiemannParams p = make_params(integrand, a, h, off, i_begin, n, coef, p0, p1, tile);
    launch_riemann_partials(p, dtype, div, {grid, kRiemannBlock}, ptr<const double>(table),
                            table_n, ptr<double>(partials), stream(s));
  };
  m.def("launch_riemann_partials",
        [partials_fn](int integrand, double a, double h, double off, uint64_t i_begin, uint64_t n,
                      std::vector<double> coef, double p0, double p1, DType dtype, DivMode div,
                      int grid, uintptr_t table, int table_n, uintptr_t partials, uintptr_t s) {
          partials_fn(integrand, a, h, off, i_begin, n, coef, p0, p1, dtype, div, grid, table,
                      table_n, partials, s, "auto");
        });
  m.def("launch_riemann_partials", partials_fn);
  // read-only views of the dispatcher (no launch): the lane tile a launch of these parameters
  // runs, and the division it runs (far sin / train angles included)
  m.def("riemann_tile_len",
        [](int integrand, double a, double h, double off, uint64_t i_begin, uint64_t n,
           std::vector<double> coef, double p0, double p1, DType dtype, DivMode div) {
          return riemann_tile_len(make_params(integrand, a, h, off, i_begin, n, coef, p0, p1),
                                  dtype, div);
        });
  m.def("riemann_tile_len",
        [](int integrand, double a, double h, double off, uint64_t i_begin, uint64_t n,
           std::vector<double> coef, double p0, double p1, DType dtype, DivMode div,
           const std::string& tile) {
          return riemann_tile_len(
              make_params(integrand, a, h, off, i_begin, n, coef, p0, p1, tile), dtype, div);
        });
  m.attr("PI4_LONG_TILE") = kSeriesHalfSpanLong * 2;
  m.def("series_ok_long", &series_ok_long);
  m.def("riemann_effective_div",
        [](int integrand, double a, double h, double off, uint64_t i_begin, uint64_t n,
           std::vector<double> coef, double p0, double p1, DType dtype, DivMode div) {
          return effective_div(make_params(integrand, a, h, off, i_begin, n, coef, p0, p1), div,
                               dtype);
        });
  m.def("riemann_pi4_ieee_narrow",
        [](int integrand, double a, double h, double off, uint64_t i_begin, uint64_t n,
           std::vector<double> coef, double p0, double p1, DType dtype) {
          return pi4_ieee_narrow(make_params(integrand, a, h, off, i_begin, n, coef, p0, p1),
                                 dtype);
        });
  // RiemannConfig::work in effect (no device needed): the plan's own resolution
  m.def("resolve_work",
        [](const std::string& work, py::object env, bool pays, bool keeps_static) {
          const std::string e = env.is_none() ? std::string() : env.cast<std::string>();
          return resolve_work(work, env.is_none() ? nullptr : e.c_str(), pays, keeps_static);
        },
        py::arg("work"), py::arg("env") = py::none(), py::arg("pays") = false,
        py::arg("keeps_static") = false);
  m.def("riemann_queue_pays",
        [](int integrand, double a, double h, double off, uint64_t i_begin, uint64_t n,
           std::vector<double> coef, double p0, double p1, DType dtype, DivMode div) {
          return riemann_queue_pays(make_params(integrand, a, h, off, i_begin, n, coef, p0, p1),
                                    dtype, div);
        });
  m.attr("TRIG_SERIES_MAX_N") = kTrigSeriesMaxN;
  m.attr("FAST_TRIG_MAX_N") = kFastTrigMaxN;
  m.attr("PI4_SERIES_MAX_X") = kPi4SeriesMaxX;
  m.attr("PI4_F32_SERIES_MAX_X") = kPi4SeriesMaxXF32;
  auto fused_fn = [](int integrand, double a, double h, double off, uint64_t i_begin, uint64_t n,
                     std::vector<double> coef, double p0, double p1, DType dtype, DivMode div,
                     int grid, uintptr_t table, int table_n, uintptr_t partials, uintptr_t ticket,
                     double scale, uintptr_t out, uintptr_t s, const std::string& tile) {
    const RiemannParams p = make_params(integrand, a, h, off, i_begin, n, coef, p0, p1, tile);
    launch_riemann_fused(p, dtype, div, {grid, kRiemannBlock}, ptr<const double>(table), table_n,
                         ptr<double>(partials), ptr<unsigned>(ticket), scale, ptr<double>(out),
                         stream(s));
  };
  m.def("launch_riemann_fused",
        [fused_fn](int integrand, double a, double h, double off, uint64_t i_begin, uint64_t n,
                   std::vector<double> coef, double p0, double p1, DType dtype, DivMode div,
                   int grid, uintptr_t table, int table_n, uintptr_t partials, uintptr_t ticket,
                   double scale, uintptr_t out, uintptr_t s) {
          fused_fn(integrand, a, h, off, i_begin, n, coef, p0, p1, dtype, div, grid, table,
                   table_n, partials, ticket, scale, out, s, "auto");
        });
  m.def("launch_riemann_fused", fused_fn);
  auto points_fn = [](int integrand, double a, double h, double off, uint64_t i_begin,
                      uint64_t n, std::vector<double> coef, double p0, double p1, DivMode div,
                      uintptr_t table, int table_n, uintptr_t out, uintptr_t s,
                      const std::string& tile) {
    const RiemannParams p = make_params(integrand, a, h, off, i_begin, n, coef, p0, p1, tile);
    launch_riemann_point_values(p, div, ptr<const double>(table), table_n, ptr<double>(out),
                                stream(s));
  };
  m.def("launch_riemann_point_values",
        [points_fn](int integrand, double a, double h, double off, uint64_t i_begin, uint64_t n,
                    std::vector<double> coef, double p0, double p1, DivMode div, uintptr_t table,
                    int table_n, uintptr_t out, uintptr_t s) {
          points_fn(integrand, a, h, off, i_begin, n, coef, p0, p1, div, table, table_n, out, s,
                    "auto");
        });
  m.def("launch_riemann_point_values", points_fn);
  m.def("launch_pi4_recip_narrow", [](uintptr_t d, uint64_t n, uintptr_t out, uintptr_t s) {
    launch_pi4_recip_narrow(ptr<const double>(d), n, ptr<double>(out), stream(s));
  });
  m.def("launch_pk_modifier_check",
        [](uintptr_t ac, uint64_t n, float ka, float kb, uintptr_t out, uintptr_t s) {
          launch_pk_modifier_check(ptr<const float>(ac), n, ka, kb, ptr<float>(out), stream(s));
        });
  m.def("launch_pi4_recip_narrow_f32", [](uintptr_t d, uint64_t n, uintptr_t out, uintptr_t s) {
    launch_pi4_recip_narrow_f32(ptr<const float>(d), n, ptr<float>(out), stream(s));
  });
  m.def("set_lds_poison", &set_lds_poison, py::arg("on"),
        "validation: staged-window kernels fill their LDS with NaN first (current device)");
  m.def("set_trig_library", &set_trig_library, py::arg("on"),
        "validation: kIeee sin/cos by ocml per sample (SinLib / TrainVelLib)");
  m.def("fast_trig_host", [](uintptr_t x, uint64_t n, int shift, uintptr_t val, uintptr_t ulp) {
    // the device's per-sample sin/cos (fast_trig.hpp, compiled for the host) and its error in
    // ulps against long double sinl/cosl; NaN value/ulp where the tile path declines
    const double* xs = reinterpret_cast<const double*>(x);
    double* v = reinterpret_cast<double*>(val);
    double* e = reinterpret_cast<double*>(ulp);
    for (uint64_t i = 0; i < n; ++i) {
      double out;
      if (!fast_trig_point(xs[i], shift, out)) {
        v[i] = e[i] = std::nan("");
        continue;
      }
      const long double ref = shift ? cosl(static_cast<long double>(xs[i]))
                                    : sinl(static_cast<long double>(xs[i]));
      const double rd = static_cast<double>(ref);
      const double sp = std::nextafter(std::fabs(rd), INFINITY) - std::fabs(rd);
      v[i] = out;
      e[i] = static_cast<double>((static_cast<long double>(out) - ref) / sp);
    }
  });
  m.def("set_pi4_library_division", &set_pi4_library_division,
        "validation: kIeee Pi4 launches use the full library division (bitwise the same sums)");
  m.def("riemann_block_ok", &riemann_block_ok);
  m.def("launch_finalize", [](uintptr_t partials, int n, double scale, uintptr_t out, uintptr_t s,
                              int block) {
    launch_finalize(ptr<const double>(partials), n, scale, ptr<double>(out), stream(s), block);
  }, py::arg("partials"), py::arg("n"), py::arg("scale"), py::arg("out"), py::arg("stream"),
     py::arg("block") = kRiemannBlock);
  m.def("default_riemann_grid", [](int cus, int waves) { return default_riemann_shape(cus, waves).grid; });
  m.def("default_reduce_grid", &default_reduce_grid);
  m.def("launch_sum_array", [](uintptr_t x, uint64_t n, double scale, uintptr_t partials, int grid,
                               uintptr_t out, uintptr_t s) {
    launch_sum_array(ptr<const double>(x), n, scale, ptr<double>(partials), grid, ptr<double>(out), stream(s));
  });
  m.def("launch_interp_fill", [](uintptr_t table, int tn, double dt, uint64_t i0, uint64_t n,
                                 uintptr_t y, uintptr_t s) {
    launch_interp_fill(ptr<const double>(table), tn, dt, i0, n, ptr<double>(y), stream(s));
  });
  m.def("scan_state_bytes", &scan_state_bytes);
  m.def("launch_inclusive_scan", [](uintptr_t in, uintptr_t out, uint64_t n, uintptr_t state,
                                    uintptr_t carry, uintptr_t s) {
    launch_inclusive_scan(ptr<const double>(in), ptr<double>(out), n, ptr<void>(state),
                          ptr<const double>(carry), stream(s));
  });
  m.def("launch_interp_scan", [](uintptr_t table, int tn, double dt, uint64_t i0, uint64_t n,
                                 uint64_t win_lo, uint64_t win_hi, uintptr_t out, uintptr_t state,
                                 uintptr_t carry, uintptr_t s) {
    launch_interp_scan_window(ptr<const double>(table), tn, dt, i0, n, win_lo, win_hi,
                              ptr<double>(out), ptr<void>(state), ptr<const double>(carry), stream(s));
  });
  m.def("scan_timeout_flag", [](uintptr_t state, uintptr_t s) { return scan_timeout_flag(ptr<const void>(state), stream(s)); });
  m.def("launch_add_carry", [](uintptr_t x, uint64_t n, uintptr_t carry, uintptr_t s) {
    launch_add_carry(ptr<double>(x), n, ptr<const double>(carry), stream(s));
  });
  m.def("table2d_grid", [](int nx, int ny, double X, double Y, int gx, int gy, int row0, int row1) {
    Table2DParams p{nullptr, nx, ny, X, Y, gx, gy, row0, row1};
    return table2d_grid(p);
  });
  m.def("table2d_path", [](int nx, int ny, double X, double Y, int gx, int gy, int row0, int row1) {
    Table2DParams p{nullptr, nx, ny, X, Y, gx, gy, row0, row1};
    return std::string(table2d_path(p));
  });
  m.def("table2d_shape_info", [](int nx, int ny, double X, double Y, int gx, int gy, int row0,
                                 int row1, int min_wg) {
    Table2DParams p{nullptr, nx, ny, X, Y, gx, gy, row0, row1, min_wg};
    const Table2DShapeInfo i = table2d_shape_info(p);
    py::dict d;
    d["stream"] = i.stream;
    d["rows_per_wave"] = i.rows_per_wave;
    d["tile_rows"] = i.tile_rows;
    d["tile_cols"] = i.tile_cols;
    d["grid"] = py::make_tuple(i.grid_x, i.grid_y);
    d["tile"] = i.tile;
    return d;
  }, py::arg("nx"), py::arg("ny"), py::arg("X"), py::arg("Y"), py::arg("gx"), py::arg("gy"),
     py::arg("row0"), py::arg("row1"), py::arg("min_wg") = 0);
  m.def("launch_table2d_partials", [](uintptr_t table, int nx, int ny, double X, double Y, int gx,
                                      int gy, int row0, int row1, uintptr_t partials, uintptr_t s) {
    Table2DParams p{ptr<const double>(table), nx, ny, X, Y, gx, gy, row0, row1};
    launch_table2d_partials(p, ptr<double>(partials), stream(s));
  });
  m.def("launch_table2d_fused", [](uintptr_t table, int nx, int ny, double X, double Y, int gx,
                                    int gy, int row0, int row1, uintptr_t partials,
                                    uintptr_t ticket, uintptr_t out, uintptr_t s) {
    Table2DParams p{ptr<const double>(table), nx, ny, X, Y, gx, gy, row0, row1};
    launch_table2d_fused(p, ptr<double>(partials), ptr<unsigned>(ticket), ptr<double>(out),
                         stream(s));
  });
  m.def("launch_table2d_chained", [](uintptr_t table, int nx, int ny, double X, double Y, int gx,
                                      int gy, int row0, int row1, uintptr_t partials,
                                      uintptr_t prev, uintptr_t prev_out, uintptr_t s) {
    Table2DParams p{ptr<const double>(table), nx, ny, X, Y, gx, gy, row0, row1};
    launch_table2d_chained(p, ptr<double>(partials), ptr<const double>(prev),
                           ptr<double>(prev_out), stream(s));
  });
  // The multi-step row stream on a caller's table (Table2DPlan runs it on its own field):
  // `steps` integrations in one launch of `phases` workgroups per block + the closing kernel;
  // partials: steps x table2d_grid doubles, outs: steps doubles.
  m.def("table2d_multistep_phases", [](int nx, int ny, double X, double Y, int gx, int gy,
                                       int row0, int row1, int min_wg, int steps, int want) {
    Table2DParams p{nullptr, nx, ny, X, Y, gx, gy, row0, row1, min_wg};
    return table2d_multistep_phases(p, 0, steps, want);
  }, py::arg("nx"), py::arg("ny"), py::arg("X"), py::arg("Y"), py::arg("gx"), py::arg("gy"),
     py::arg("row0"), py::arg("row1"), py::arg("min_wg"), py::arg("steps"), py::arg("want") = 0);
  m.def("launch_table2d_multistep", [](uintptr_t table, int nx, int ny, double X, double Y,
                                        int gx, int gy, int row0, int row1, int min_wg,
                                        uintptr_t partials, int steps, uintptr_t outs,
                                        uintptr_t s, int phases) {
    Table2DParams p{ptr<const double>(table), nx, ny, X, Y, gx, gy, row0, row1, min_wg};
    launch_table2d_multistep(p, ptr<double>(partials), steps, ptr<double>(outs), stream(s),
                             phases);
  }, py::arg("table"), py::arg("nx"), py::arg("ny"), py::arg("X"), py::arg("Y"), py::arg("gx"),
     py::arg("gy"), py::arg("row0"), py::arg("row1"), py::arg("min_wg"), py::arg("partials"),
     py::arg("steps"), py::arg("outs"), py::arg("stream"), py::arg("phases") = 1);
  m.def("launch_table2d_finalize", [](uintptr_t partials, int n, uintptr_t out, uintptr_t s) {
    launch_table2d_finalize(ptr<const double>(partials), n, ptr<double>(out), stream(s));
  });
  m.def("launch_outer_product", [](uintptr_t v, int n, uintptr_t t, uintptr_t s) {
    launch_outer_product(ptr<const double>(v), n, ptr<double>(t), stream(s));
  });
  m.def("selftest_wave_ops", [](uintptr_t in, uint64_t n, bool f32, uintptr_t sums, uintptr_t scan, uintptr_t s) {
    selftest_wave_ops(ptr<const void>(in), n, f32, ptr<void>(sums), ptr<void>(scan), stream(s));
  });
  m.def("selftest_block_ops", [](uintptr_t in, uint64_t n, int block, bool f32, uintptr_t sums,
                                 uintptr_t scan, uintptr_t s) {
    selftest_block_ops(ptr<const void>(in), n, block, f32, ptr<void>(sums), ptr<void>(scan), stream(s));
  });

  // ------------------------------------------------------------------ train scan pipeline
  py::class_<TrainScanConfig>(m, "TrainScanConfig")
      .def(py::init<>())
      .def_readwrite("steps_per_sec", &TrainScanConfig::steps_per_sec)
      .def_readwrite("seconds", &TrainScanConfig::seconds)
      .def_readwrite("parity", &TrainScanConfig::parity)
      .def_readwrite("replicate", &TrainScanConfig::replicate)
      .def_readwrite("phase2", &TrainScanConfig::phase2)
      .def_readwrite("table", &TrainScanConfig::table)
      .def_property("algo", [](const TrainScanConfig& c) { return scan_algo_name(c.algo); },
                    [](TrainScanConfig& c, const std::string& s) {
                      c.algo = scan_algo_of(s);
                    });
  m.def("trainscan_workspace_bytes", &trainscan_workspace_bytes);
  // the --replicate fingerprint (host code): FNV-1a over the fp64 bits, compensated sum,
  // elements at 0, n/4, n/2, 3n/4, n-1
  m.def("replica_digest", [](const std::vector<double>& v) {
    const ReplicaDigest d = digest_table(v.data(), v.size());
    py::dict r;
    r["hash"] = d.hash;
    r["n"] = d.n;
    r["sum"] = d.sum;
    r["at"] = std::vector<double>(d.at, d.at + 5);
    return r;
  });

  // ------------------------------------------------------------------ 2-D field plan
  py::class_<Table2DPlan>(m, "Table2DPlan")
      .def(py::init([](int grid, double extent, int device, const Comm* comm, bool bucket,
                       bool chain, int step_streams, int slice_rank, int slice_world,
                       bool multistep, int phases, int min_wg, int graph_steps,
                       bool force_collective) {
             Table2DConfig c;
             c.force_collective = force_collective;
             c.graph_steps = graph_steps;
             c.phases = phases;
             c.min_wg = min_wg;
             c.grid = grid;
             c.extent = extent;
             c.bucket = bucket;
             c.chain = chain;
             c.step_streams = step_streams;
             c.multistep = multistep;
             c.rank = slice_rank;   // without a communicator: that rank's rows only
             c.world = slice_world;
             return new Table2DPlan(c, device, comm);
           }),
           py::arg("grid") = 4096, py::arg("extent") = 1800.0, py::arg("device") = 0,
           py::arg("comm") = nullptr, py::arg("bucket") = true, py::arg("chain") = true,
           py::arg("step_streams") = 0, py::arg("slice_rank") = 0, py::arg("slice_world") = 1,
           py::arg("multistep") = true, py::arg("phases") = 0, py::arg("min_wg") = 0,
           py::arg("graph_steps") = 0, py::arg("force_collective") = false,
           py::keep_alive<1, 5>())
      .def_property_readonly("phases", &Table2DPlan::phases)
      .def_property_readonly("min_wg", &Table2DPlan::min_wg)
      .def_property_readonly("workgroups", &Table2DPlan::workgroups)
      .def_property_readonly("resident_per_cu", &Table2DPlan::resident_per_cu)
      .def_property_readonly("step_streams",
                             [](const Table2DPlan& p) { return p.step_streams(); })
      .def_property_readonly("multistep", &Table2DPlan::multistep)
      .def("run", &Table2DPlan::run, py::call_guard<py::gil_scoped_release>())
      .def("time", &Table2DPlan::time, py::arg("iters"), py::arg("graphs") = true,
           py::call_guard<py::gil_scoped_release>())
      .def("last_result", &Table2DPlan::last_result)
      .def_property_readonly("bucketed", &Table2DPlan::bucketed)
      .def_property_readonly("chained", &Table2DPlan::chained)
      .def_property_readonly("collective", &Table2DPlan::collective)
      .def_property_readonly("graph_steps", &Table2DPlan::graph_steps)
      .def_property_readonly("row0", &Table2DPlan::row0)
      .def_property_readonly("row1", &Table2DPlan::row1);
  m.def("table2d_oracle", &table2d_oracle, py::arg("grid"), py::arg("extent") = 1800.0);
  m.def("table2d_auto_graph_steps", &table2d_auto_graph_steps, py::arg("grid"),
        py::arg("extent") = 1800.0, py::arg("world") = 1);
  m.def("launch_trainscan", [](uintptr_t table, int tn, double dt, uint64_t i0, uint64_t n,
                               uint64_t win_lo, uint64_t win_hi, uintptr_t ws, uintptr_t totals,
                               uintptr_t carries, uintptr_t vel, uintptr_t pos, uintptr_t s,
                               bool fold) {
    // fold = true: the one-GPU form TrainScan::enqueue_fused runs (per-workgroup fold of the
    // block aggregates, totals not written) where it applies, else the hand-off as before
    TrainScanKernelParams p{ptr<const double>(table), tn, dt, i0, n, win_lo, win_hi};
    launch_trainscan_local(p, ptr<void>(ws), ptr<double>(totals), stream(s), fold);
    launch_trainscan_write(p, ptr<const void>(ws), ptr<const double>(carries), ptr<double>(vel),
                           ptr<double>(pos), stream(s), fold);
  }, py::arg("table"), py::arg("table_n"), py::arg("dt"), py::arg("i0"), py::arg("n"),
     py::arg("win_lo"), py::arg("win_hi"), py::arg("ws"), py::arg("totals"), py::arg("carries"),
     py::arg("vel"), py::arg("pos"), py::arg("stream"), py::arg("fold") = false);
  m.def("trainscan_fold_applies", [](double dt, uint64_t n) {
    TrainScanKernelParams p{nullptr, 2, dt, 0, n, 0, ~uint64_t(0)};
    return trainscan_fold_applies(p);
  }, "does launch_trainscan(fold = true) take the fold variant for this dt and slice length?");
  m.def("launch_trainscan_onepass", [](uintptr_t table, int tn, double dt, uint64_t i0,
                                       uint64_t n, uint64_t win_lo, uint64_t win_hi, uintptr_t ws,
                                       uintptr_t totals, uintptr_t vel, uintptr_t pos,
                                       uintptr_t s) {
    TrainScanKernelParams p{ptr<const double>(table), tn, dt, i0, n, win_lo, win_hi};
    launch_trainscan_onepass(p, ptr<void>(ws), ptr<double>(vel), ptr<double>(pos),
                             ptr<double>(totals), stream(s));
  });
  m.def("trainscan_onepass_timeout", [](uintptr_t ws, uintptr_t s) {
    return trainscan_onepass_timeout(ptr<const void>(ws), stream(s));
  });
  py::class_<TrainScan>(m, "TrainScan")
      .def(py::init<const TrainScanConfig&, int, const Comm*>(), py::arg("config"),
           py::arg("device"), py::arg("comm") = nullptr, py::keep_alive<1, 4>())
      .def("run", [](TrainScan& t) {
        TrainScanResult r;
        {
          py::gil_scoped_release nogil;
          r = t.run();
        }
        py::dict d;
        d["distance"] = r.distance;
        d["sum_of_sums"] = r.sum_of_sums;
        d["distance_scan"] = r.distance_scan;
        d["device_ms"] = r.device_ms;
        d["timeout"] = r.timeout;
        return d;
      })
      .def_property_readonly("local_begin", &TrainScan::local_begin)
      .def_property_readonly("algo", [](const TrainScan& t) { return scan_algo_name(t.algo()); })
      .def_property_readonly("local_count", &TrainScan::local_count)
      .def("velocity_ptr", [](const TrainScan& t) { return reinterpret_cast<uintptr_t>(t.velocity()); })
      .def("position_ptr", [](const TrainScan& t) { return reinterpret_cast<uintptr_t>(t.position()); })
      .def("replicated_ptr", [](const TrainScan& t) { return reinterpret_cast<uintptr_t>(t.replicated()); })
      .def_property_readonly("total", &TrainScan::total);

  // ------------------------------------------------------------------ runtime integrands
  m.def("expr_source", &expr_source, "kernel source generated for an expression over x");
  m.def("expr_compile", compiled(&expr_compile),
        "compile an expression for gfx950 with hipRTC (no device needed); the code object");
  py::class_<ExprIntegrator>(m, "ExprIntegrator",
                             "f(x) given as an expression, compiled with hipRTC for gfx950")
      .def(py::init<const std::string&, int, int>(), py::arg("expr"), py::arg("device") = 0,
           py::arg("grid") = 2048)
      .def("integrate", &ExprIntegrator::integrate, py::arg("a"), py::arg("b"), py::arg("n"),
           py::arg("rule"), py::arg("begin"), py::arg("count"), py::arg("scale") = 1.0,
           py::arg("comm") = nullptr, py::call_guard<py::gil_scoped_release>())
      .def("time",
           [](ExprIntegrator& e, double a, double b, uint64_t n, Rule rule, uint64_t begin,
              uint64_t count, int iters) { return e.time(a, b, n, rule, begin, count, iters); },
           py::arg("a"), py::arg("b"), py::arg("n"), py::arg("rule"), py::arg("begin"),
           py::arg("count"), py::arg("iters"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("expression", &ExprIntegrator::expression);

  // parameter sweeps: f(x, p0..p7) over K rows per launch
  m.def("expr_sweep_source", &expr_sweep_source, py::arg("expr"), py::arg("nparams"),
        "kernel source generated for an expression over x and p0..p{nparams-1}");
  m.def("expr_sweep_compile", compiled(&expr_sweep_compile),
        py::arg("expr"), py::arg("nparams"),
        "compile a sweep expression for gfx950 with hipRTC (no device needed); the code object");
  m.attr("SWEEP_MAX_GRID") = kSweepMaxGrid;
  m.attr("SWEEP_MAX_PARTIALS") = kSweepMaxPartials;
  m.def("expr_sweep_shape", [](uint64_t n_local, uint64_t rows, int grid) {
          const SweepShape s = expr_sweep_shape(n_local, rows, grid);
          return py::make_tuple(s.gx, s.gy);
        },
        py::arg("n_local"), py::arg("rows"), py::arg("grid") = 0,
        "(gx, gy) of a sweep launch; gx never depends on rows");
  m.def("load_param_rows", [](const std::string& path) {
          int np = 0;
          std::vector<double> v = load_param_rows(path, &np);
          const py::ssize_t rows = np ? static_cast<py::ssize_t>(v.size()) / np : 0;
          py::array_t<double> a({rows, static_cast<py::ssize_t>(np)});
          std::copy(v.begin(), v.end(), a.mutable_data());
          return a;
        },
        py::arg("path"), "parameter rows of a text file as a 2-D float64 array");
  m.def("linspace_param_rows", [](const std::string& spec) {
          std::vector<double> v = linspace_param_rows(spec);
          py::array_t<double> a({static_cast<py::ssize_t>(v.size()), py::ssize_t(1)});
          std::copy(v.begin(), v.end(), a.mutable_data());
          return a;
        },
        py::arg("spec"), "p0=LO:HI:COUNT as a COUNT x 1 float64 array");
  py::class_<ExprSweep>(m, "ExprSweep",
                        "f(x, p0..p7) as an expression: K parameter rows per launch (hipRTC)")
      .def(py::init<const std::string&, int, int, int>(), py::arg("expr"), py::arg("nparams"),
           py::arg("device") = 0, py::arg("grid") = 0)
      .def("integrate",
           [](ExprSweep& e, const ParamRows& params, double a, double b, uint64_t n, Rule rule,
              uint64_t begin, uint64_t count, double scale, const Comm* comm) {
             uint64_t rows = 0;
             const std::vector<double> p = param_rows(params, e.nparams(), &rows);
             std::vector<double> v;
             {
               py::gil_scoped_release nogil;
               v = e.integrate(p, rows, a, b, n, rule, begin, count, scale, comm);
             }
             return py::array_t<double>(static_cast<py::ssize_t>(v.size()), v.data());
           },
           py::arg("params"), py::arg("a"), py::arg("b"), py::arg("n"), py::arg("rule"),
           py::arg("begin"), py::arg("count"), py::arg("scale") = 1.0,
           py::arg("comm") = nullptr)
      .def("time",
           [](ExprSweep& e, const ParamRows& params, double a, double b, uint64_t n, Rule rule,
              uint64_t begin, uint64_t count, int iters) {
             uint64_t rows = 0;
             const std::vector<double> p = param_rows(params, e.nparams(), &rows);
             py::gil_scoped_release nogil;
             return e.time(p, rows, a, b, n, rule, begin, count, iters);
           },
           py::arg("params"), py::arg("a"), py::arg("b"), py::arg("n"), py::arg("rule"),
           py::arg("begin"), py::arg("count"), py::arg("iters"))
      .def_property_readonly("expression", &ExprSweep::expression)
      .def_property_readonly("nparams", &ExprSweep::nparams);

  // running integrals: F_i = scale * h * sum_{j <= i} f(x_j) on the sample grid
  m.attr("EXPR_SCAN_TILE") = EXPR_SCAN_TILE;
  m.attr("EXPR_SCAN_MAX_TILES") = kExprScanMaxTiles;
  m.def("expr_scan_source", &expr_scan_source, py::arg("expr"),
        "source of the running-integral kernels generated for an expression over x");
  m.def("expr_scan_compile", compiled(&expr_scan_compile),
        py::arg("expr"),
        "compile the running-integral kernels for gfx950 with hipRTC (no device needed)");
  m.def("expr_scan_shape", [](uint64_t count) {
          const ScanShape s = expr_scan_shape(count);
          return py::make_tuple(s.tiles, s.run, s.runs);
        },
        py::arg("count"), "(tiles, tiles per run, runs) of a scan of `count` samples");
  m.def("expr_scan_outputs", &expr_scan_outputs, py::arg("begin"), py::arg("count"),
        py::arg("every"), "values a scan of samples [begin, begin + count) writes");
  m.def("expr_scan_check", &expr_scan_check, py::arg("n"), py::arg("begin"), py::arg("count"),
        py::arg("every"), py::arg("out_capacity"),
        "raise unless the slice, `every` and the output capacity are ones a scan accepts");
  py::class_<ExprScan>(m, "ExprScan",
                       "running integral of f(x) given as an expression (hipRTC, gfx950)")
      .def(py::init<const std::string&, int>(), py::arg("expr"), py::arg("device") = 0)
      .def("run",
           [](ExprScan& e, double a, double b, uint64_t n, Rule rule, uint64_t begin,
              uint64_t count, uint64_t every, uintptr_t out, uint64_t out_capacity, double scale,
              const Comm* comm) {
             ExprScanResult r;
             {
               py::gil_scoped_release nogil;  // loopback collectives barrier across threads
               r = e.run(a, b, n, rule, begin, count, every, reinterpret_cast<double*>(out),
                         out_capacity, scale, comm);
             }
             py::dict d;
             d["total"] = r.total;
             d["outputs"] = r.outputs;
             d["device_ms"] = r.device_ms;
             return d;
           },
           py::arg("a"), py::arg("b"), py::arg("n"), py::arg("rule"), py::arg("begin"),
           py::arg("count"), py::arg("every"), py::arg("out"), py::arg("out_capacity"),
           py::arg("scale") = 1.0, py::arg("comm") = nullptr)
      .def("time",
           [](ExprScan& e, double a, double b, uint64_t n, Rule rule, uint64_t begin,
              uint64_t count, uint64_t every, uintptr_t out, uint64_t out_capacity, int iters) {
             return e.time(a, b, n, rule, begin, count, every, reinterpret_cast<double*>(out),
                           out_capacity, iters);
           },
           py::arg("a"), py::arg("b"), py::arg("n"), py::arg("rule"), py::arg("begin"),
           py::arg("count"), py::arg("every"), py::arg("out"), py::arg("out_capacity"),
           py::arg("iters"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("expression", &ExprScan::expression);

  // double integrals: f(x, y) over the nx x ny samples of a rectangle
  m.attr("EXPR2D_MAX_NX") = kExpr2DMaxNx;
  m.attr("EXPR2D_MAX_NY") = kExpr2DMaxNy;
  m.attr("EXPR2D_MAX_GRID") = kExpr2DMaxGrid;
  m.def("expr2d_source", &expr2d_source, py::arg("expr"),
        "kernel source generated for an expression over x and y");
  m.def("expr2d_compile", compiled(&expr2d_compile),
        py::arg("expr"),
        "compile a 2-D expression for gfx950 with hipRTC (no device needed); the code object");
  py::class_<Expr2DShape>(m, "Expr2DShape", "how a 2-D launch is dealt out (expr2d_shape)")
      .def_readonly("lanes_x", &Expr2DShape::lanes_x)
      .def_readonly("cols_per_lane", &Expr2DShape::cols_per_lane)
      .def_readonly("rows_per_item", &Expr2DShape::rows_per_item)
      .def_readonly("stretches", &Expr2DShape::stretches)
      .def_readonly("panels", &Expr2DShape::panels)
      .def_readonly("items", &Expr2DShape::items)
      .def_readonly("items_per_wg", &Expr2DShape::items_per_wg)
      .def_readonly("workgroups", &Expr2DShape::workgroups)
      .def_readonly("lane_samples", &Expr2DShape::lane_samples)
      .def("as_tuple", [](const Expr2DShape& s) {
        return py::make_tuple(s.lanes_x, s.cols_per_lane, s.rows_per_item, s.items,
                              s.items_per_wg, s.workgroups);
      }, "(lanes along x, columns per lane, rows per item, items, items per workgroup, "
         "workgroups)");
  m.def("expr2d_shape", &expr2d_shape, py::arg("nx"), py::arg("row_count"), py::arg("grid") = 0,
        "launch shape of all nx columns of row_count rows: a function of these three only");
  m.def("expr2d_check", &expr2d_check, py::arg("nx"), py::arg("ny"), py::arg("row_begin"),
        py::arg("row_count"), py::arg("grid") = 0,
        "raise unless the rule and the row slice are ones a 2-D launch accepts");
  m.def("expr2d_plan", &expr2d_plan, py::arg("nx"), py::arg("ny"), py::arg("row_begin"),
        py::arg("row_count"), py::arg("grid") = 0,
        "expr2d_check, then the shape ExprIntegrator2D launches that slice with");
  m.def("fma_coords", [](uint64_t first, uint64_t count, double off, double h, double a) {
          py::array_t<double> out(static_cast<py::ssize_t>(count));
          double* p = out.mutable_data();
          for (uint64_t i = 0; i < count; ++i)
            p[i] = std::fma(static_cast<double>(first + i) + off, h, a);
          return out;
        },
        py::arg("first"), py::arg("count"), py::arg("off"), py::arg("h"), py::arg("a"),
        "fma((double)i + off, h, a) for i in [first, first + count): the coordinates the "
        "expression kernels form, rounded once");
  py::class_<ExprIntegrator2D>(m, "ExprIntegrator2D",
                               "f(x, y) as an expression over a rectangle (hipRTC, gfx950)")
      .def(py::init<const std::string&, int, int>(), py::arg("expr"), py::arg("device") = 0,
           py::arg("grid") = 0)
      .def("integrate", &ExprIntegrator2D::integrate, py::arg("ax"), py::arg("bx"),
           py::arg("nx"), py::arg("ay"), py::arg("by"), py::arg("ny"), py::arg("rule"),
           py::arg("row_begin"), py::arg("row_count"), py::arg("scale") = 1.0,
           py::arg("comm") = nullptr, py::call_guard<py::gil_scoped_release>())
      .def("time",
           [](ExprIntegrator2D& e, double ax, double bx, uint64_t nx, double ay, double by,
              uint64_t ny, Rule rule, uint64_t row_begin, uint64_t row_count, int iters) {
             return e.time(ax, bx, nx, ay, by, ny, rule, row_begin, row_count, iters);
           },
           py::arg("ax"), py::arg("bx"), py::arg("nx"), py::arg("ay"), py::arg("by"),
           py::arg("ny"), py::arg("rule"), py::arg("row_begin"), py::arg("row_count"),
           py::arg("iters"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("expression", &ExprIntegrator2D::expression);

  // adaptive integration: Gauss-Kronrod (7, 15), bisection by rounds, to a tolerance
  m.attr("ADAPT_MAX_INTERVALS_LIMIT") = kAdaptMaxIntervalsLimit;
  m.attr("ADAPT_MAX_DEPTH_LIMIT") = kAdaptMaxDepthLimit;
  m.attr("ADAPT_DEFAULT_PANELS") = kAdaptDefaultPanels;
  auto as_array = [](const std::vector<double>& v) {
    return py::array_t<double>(static_cast<py::ssize_t>(v.size()), v.data());
  };
  m.def("gk15_nodes", [as_array] { return as_array(gk15_nodes()); },
        "the 15 Kronrod nodes on [-1, 1], ascending (the rule's own table)");
  m.def("gk15_weights", [as_array] { return as_array(gk15_weights()); },
        "the weights of gk15_nodes()");
  m.def("gk7_weights", [as_array] { return as_array(gk7_weights()); },
        "the weights of the 7 Gauss nodes, which are nodes 1, 3, ..., 13 of gk15_nodes()");
  m.def("gk15_abscissae",
        [](py::array_t<double, py::array::c_style | py::array::forcecast> lo,
           py::array_t<double, py::array::c_style | py::array::forcecast> hi) {
          MIINT_CHECK(lo.ndim() == 1 && hi.ndim() == 1 && lo.shape(0) == hi.shape(0),
                      "gk15_abscissae: lo and hi are 1-D arrays of one length");
          const py::ssize_t n = lo.shape(0);
          py::array_t<double> out({n, py::ssize_t(15)});
          for (py::ssize_t i = 0; i < n; ++i)
            gk15_abscissae(lo.data()[i], hi.data()[i], out.mutable_data() + 15 * i);
          return out;
        },
        py::arg("lo"), py::arg("hi"),
        "the nodes fma(hw, t_j, c) of every interval [lo_i, hi_i] as an n x 15 array: the bits "
        "the adaptive kernels evaluate f at");
  py::class_<AdaptOptions>(m, "AdaptOptions", "tolerances and bounds of an adaptive integration")
      .def(py::init([](double rtol, double atol, uint64_t panels, int max_depth,
                       uint64_t max_intervals, bool unbounded) {
             AdaptOptions o;
             o.rtol = rtol;
             o.atol = atol;
             o.panels = panels;
             o.max_depth = max_depth;
             o.max_intervals = max_intervals;
             o.unbounded = unbounded;
             return o;
           }),
           py::arg("rtol") = 1e-10, py::arg("atol") = 0.0, py::arg("panels") = kAdaptDefaultPanels,
           py::arg("max_depth") = 60, py::arg("max_intervals") = uint64_t(1) << 22,
           py::arg("unbounded") = false)
      .def_readwrite("unbounded", &AdaptOptions::unbounded)
      .def_readwrite("rtol", &AdaptOptions::rtol)
      .def_readwrite("atol", &AdaptOptions::atol)
      .def_readwrite("panels", &AdaptOptions::panels)
      .def_readwrite("max_depth", &AdaptOptions::max_depth)
      .def_readwrite("max_intervals", &AdaptOptions::max_intervals);
  py::class_<AdaptResult>(m, "AdaptResult", "value, error estimate and counters of one call")
      .def_readonly("value", &AdaptResult::value)
      .def_readonly("err_est", &AdaptResult::err_est)
      .def_readonly("resabs", &AdaptResult::resabs)
      .def_readonly("tol", &AdaptResult::tol)
      .def_readonly("converged", &AdaptResult::converged)
      .def_readonly("evals", &AdaptResult::evals)
      .def_readonly("rounds", &AdaptResult::rounds)
      .def_readonly("intervals", &AdaptResult::intervals)
      .def_readonly("splits", &AdaptResult::splits)
      .def_readonly("floor", &AdaptResult::floor)
      .def_readonly("forced", &AdaptResult::forced)
      .def_readonly("nonfinite", &AdaptResult::nonfinite)
      .def_readonly("capped", &AdaptResult::capped)
      .def_readonly("device_ms", &AdaptResult::device_ms)
      .def_readonly("range", &AdaptResult::range)
      .def("as_dict", [](const AdaptResult& r) {
        py::dict d;
        d["value"] = r.value;
        d["err_est"] = r.err_est;
        d["resabs"] = r.resabs;
        d["tol"] = r.tol;
        d["converged"] = r.converged;
        d["evals"] = r.evals;
        d["rounds"] = r.rounds;
        d["intervals"] = r.intervals;
        d["splits"] = r.splits;
        d["floor"] = r.floor;
        d["forced"] = r.forced;
        d["nonfinite"] = r.nonfinite;
        d["capped"] = r.capped;
        d["device_ms"] = r.device_ms;
        d["range"] = r.range;
        return d;
      });
  m.def("adapt_range",
        [](double a, double b) { return std::string(adapt_range_name(adapt_range(a, b))); },
        py::arg("a"), py::arg("b"),
        "'finite', 'upper', 'lower' or 'both': the kind of the range between a and b");
  m.def("adapt_range_map",
        [](double a, double b, py::array_t<double, py::array::c_style | py::array::forcecast> t) {
          MIINT_CHECK(t.ndim() == 1, "adapt_range_map: t is a 1-D array");
          const py::ssize_t n = t.shape(0);
          py::array_t<double> x(n), jac(n), x2(n);
          adapt_range_map(a, b, t.data(), static_cast<uint64_t>(n), x.mutable_data(),
                          jac.mutable_data(), x2.mutable_data());
          return py::make_tuple(x, jac, x2);
        },
        py::arg("a"), py::arg("b"), py::arg("t"),
        "the map of an infinite range at every t in (0, 1], in the bits the kernels form: "
        "(x, jac, x2) with q = (1 - t) / t, jac = t * t and x = a + q (upper), b - q (lower) or "
        "x = q, x2 = -q (both; x2 = x otherwise): g(t) = f(x) / jac, or (f(x) + f(x2)) / jac");
  m.def("expr_adapt_unbounded_source", &expr_adapt_unbounded_source, py::arg("expr"),
        "source of the eval kernels of the infinite kinds for an expression over x");
  m.def("expr_adapt_unbounded_compile", compiled(&expr_adapt_unbounded_compile), py::arg("expr"),
        "compile the unbounded eval kernels for gfx950 with hipRTC (no device needed)");
  m.def("adapt_check", &adapt_check, py::arg("a"), py::arg("b"), py::arg("options"),
        "raise, naming the numbers, unless the range and the options are ones ExprAdaptive takes");
  m.def("expr_adapt_source", &expr_adapt_source, py::arg("expr"),
        "source of the adaptive kernels generated for an expression over x");
  m.def("expr_adapt_compile", compiled(&expr_adapt_compile), py::arg("expr"),
        "compile the adaptive kernels for gfx950 with hipRTC (no device needed)");
  py::class_<ExprAdaptive>(m, "ExprAdaptive",
                           "the integral of f(x) to a requested tolerance (hipRTC, gfx950)")
      .def(py::init<const std::string&, int>(), py::arg("expr"), py::arg("device") = 0)
      .def("integrate",
           [](ExprAdaptive& e, double a, double b, const AdaptOptions& o, uintptr_t out,
              uint64_t capacity) {
             return e.integrate(a, b, o, reinterpret_cast<double*>(out), capacity);
           },
           py::arg("a"), py::arg("b"), py::arg("options") = AdaptOptions(),
           py::arg("intervals_out") = 0, py::arg("capacity") = 0,
           py::call_guard<py::gil_scoped_release>())
      .def("time", &ExprAdaptive::time, py::arg("a"), py::arg("b"), py::arg("options"),
           py::arg("iters"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("expression", &ExprAdaptive::expression);

  // oscillatory weights: Filon-Clenshaw-Curtis (13, 25) against cos(omega x) or sin(omega x)
  m.attr("OSC_ROW") = kOscRow;
  m.def("osc_nodes", [as_array] { return as_array(osc_nodes()); },
        "the 25 Chebyshev extrema cos(j pi / 24), j = 0 .. 24, descending");
  m.def("osc_cc_weights", [as_array] { return as_array(osc_cc_weights()); },
        "the plain Clenshaw-Curtis weights of osc_nodes()");
  m.def("osc_weights",
        [as_array](double par) {
          const std::vector<double> w = osc_weights(par);
          auto part = [&](size_t from, size_t count) {
            return as_array(std::vector<double>(w.begin() + from, w.begin() + from + count));
          };
          return py::make_tuple(part(0, 25), part(25, 25), part(50, 13), part(63, 13));
        },
        py::arg("par"),
        "(Wc24, Ws24, Wc12, Ws12): the integrals of the Lagrange basis on the 25 (13) Chebyshev "
        "extrema against cos(par t) and sin(par t) over [-1, 1], the doubles the device table holds");
  m.def("osc_table_row",
        [as_array](double par) {
          std::vector<double> row(kOscRow);
          osc_table_row(par, row.data());
          return as_array(row);
        },
        py::arg("par"), "a depth's row of the device table: the half tables");
  m.def("osc_abscissae",
        [](py::array_t<double, py::array::c_style | py::array::forcecast> lo,
           py::array_t<double, py::array::c_style | py::array::forcecast> hi) {
          MIINT_CHECK(lo.ndim() == 1 && hi.ndim() == 1 && lo.shape(0) == hi.shape(0),
                      "osc_abscissae: lo and hi are 1-D arrays of one length");
          const py::ssize_t n = lo.shape(0);
          py::array_t<double> out({n, py::ssize_t(25)});
          for (py::ssize_t i = 0; i < n; ++i)
            osc_abscissae(lo.data()[i], hi.data()[i], out.mutable_data() + 25 * i);
          return out;
        },
        py::arg("lo"), py::arg("hi"),
        "the nodes of every interval [lo_i, hi_i] as an n x 25 array in the order of osc_nodes(): "
        "the bits the oscillatory kernels evaluate f at");
  m.def("osc_epsilon",
        [](py::array_t<double, py::array::c_style | py::array::forcecast> s) {
          MIINT_CHECK(s.ndim() == 1, "osc_epsilon: s is a 1-D array");
          return osc_epsilon(s.data(), static_cast<int>(s.shape(0)));
        },
        py::arg("s"), "Wynn's epsilon algorithm on the partial sums s (at least 3)");
  py::class_<OscTailOptions>(m, "OscTailOptions", "the Fourier tail's cycles")
      .def(py::init([](uint64_t panels, int max_cycles) {
             OscTailOptions o;
             o.panels = panels;
             o.max_cycles = max_cycles;
             return o;
           }),
           py::arg("panels") = 16, py::arg("max_cycles") = 50)
      .def_readwrite("panels", &OscTailOptions::panels)
      .def_readwrite("max_cycles", &OscTailOptions::max_cycles);
  py::class_<OscResult, AdaptResult>(m, "OscResult",
                                     "AdaptResult and omega, kind, cycles, extrapolated, reason")
      .def_readonly("omega", &OscResult::omega)
      .def_readonly("kind", &OscResult::kind)
      .def_readonly("cycles", &OscResult::cycles)
      .def_readonly("extrapolated", &OscResult::extrapolated)
      .def_readonly("reason", &OscResult::reason)
      .def("as_dict", [](const OscResult& r) {
        py::dict d;
        d["value"] = r.value;
        d["err_est"] = r.err_est;
        d["resabs"] = r.resabs;
        d["tol"] = r.tol;
        d["converged"] = r.converged;
        d["evals"] = r.evals;
        d["rounds"] = r.rounds;
        d["intervals"] = r.intervals;
        d["splits"] = r.splits;
        d["floor"] = r.floor;
        d["forced"] = r.forced;
        d["nonfinite"] = r.nonfinite;
        d["capped"] = r.capped;
        d["device_ms"] = r.device_ms;
        d["range"] = r.range;
        d["omega"] = r.omega;
        d["kind"] = r.kind;
        d["cycles"] = r.cycles;
        d["extrapolated"] = r.extrapolated;
        d["reason"] = r.reason;
        return d;
      });
  m.def("osc_check",
        [](double a, double b, double omega, const AdaptOptions& o, bool tail,
           const OscTailOptions& t) { osc_check(a, b, omega, o, tail, t); },
        py::arg("a"), py::arg("b"), py::arg("omega"), py::arg("options"),
        py::arg("tail") = false, py::arg("tail_options") = OscTailOptions(),
        "raise, naming the numbers, unless ExprAdaptiveOsc takes the range, omega and options");
  m.def("expr_osc_source", &expr_osc_source, py::arg("expr"),
        "source of the two oscillatory eval kernels generated for an expression over x");
  m.def("expr_osc_compile", compiled(&expr_osc_compile), py::arg("expr"),
        "compile the oscillatory eval kernels for gfx950 with hipRTC (no device needed)");
  py::class_<ExprAdaptiveOsc>(m, "ExprAdaptiveOsc",
                              "the integral of f(x) cos(omega x) or f(x) sin(omega x) to a "
                              "requested tolerance (hipRTC, gfx950)")
      .def(py::init<const std::string&, int>(), py::arg("expr"), py::arg("device") = 0)
      .def("integrate",
           [](ExprAdaptiveOsc& e, double a, double b, double omega, const std::string& kind,
              const AdaptOptions& o, uintptr_t out, uint64_t capacity) {
             return e.integrate(a, b, omega, osc_kind(kind), o, reinterpret_cast<double*>(out),
                                capacity);
           },
           py::arg("a"), py::arg("b"), py::arg("omega"), py::arg("kind") = "cos",
           py::arg("options") = AdaptOptions(), py::arg("intervals_out") = 0,
           py::arg("capacity") = 0, py::call_guard<py::gil_scoped_release>())
      .def("integrate_tail",
           [](ExprAdaptiveOsc& e, double a, double omega, const std::string& kind,
              const AdaptOptions& o, const OscTailOptions& t) {
             return e.integrate_tail(a, omega, osc_kind(kind), o, t);
           },
           py::arg("a"), py::arg("omega"), py::arg("kind") = "cos",
           py::arg("options") = AdaptOptions(), py::arg("tail_options") = OscTailOptions(),
           py::call_guard<py::gil_scoped_release>())
      .def("time",
           [](ExprAdaptiveOsc& e, double a, double b, double omega, const std::string& kind,
              const AdaptOptions& o, int iters) {
             return e.time(a, b, omega, osc_kind(kind), o, iters);
           },
           py::arg("a"), py::arg("b"), py::arg("omega"), py::arg("kind"), py::arg("options"),
           py::arg("iters"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("table_uploads", &ExprAdaptiveOsc::table_uploads)
      .def_property_readonly("expression", &ExprAdaptiveOsc::expression);

  // adaptive double integrals: the (7, 15) x (7, 15) product on rectangles bisected by rounds
  m.attr("ADAPT2D_DEFAULT_PANELS") = kAdapt2DDefaultPanels;
  py::class_<Adapt2DOptions>(m, "Adapt2DOptions",
                             "tolerances and bounds of an adaptive double integral")
      .def(py::init([](double rtol, double atol, uint64_t panels_x, uint64_t panels_y,
                       int max_depth, uint64_t max_intervals) {
             Adapt2DOptions o;
             o.rtol = rtol;
             o.atol = atol;
             o.panels_x = panels_x;
             o.panels_y = panels_y;
             o.max_depth = max_depth;
             o.max_intervals = max_intervals;
             return o;
           }),
           py::arg("rtol") = 1e-10, py::arg("atol") = 0.0,
           py::arg("panels_x") = kAdapt2DDefaultPanels,
           py::arg("panels_y") = kAdapt2DDefaultPanels, py::arg("max_depth") = 60,
           py::arg("max_intervals") = uint64_t(1) << 22)
      .def_readwrite("rtol", &Adapt2DOptions::rtol)
      .def_readwrite("atol", &Adapt2DOptions::atol)
      .def_readwrite("panels_x", &Adapt2DOptions::panels_x)
      .def_readwrite("panels_y", &Adapt2DOptions::panels_y)
      .def_readwrite("max_depth", &Adapt2DOptions::max_depth)
      .def_readwrite("max_intervals", &Adapt2DOptions::max_intervals);
  py::class_<Adapt2DResult>(m, "Adapt2DResult", "value, error estimate and counters of one call")
      .def(py::init<>())
      .def_readonly("value", &Adapt2DResult::value)
      .def_readonly("err_est", &Adapt2DResult::err_est)
      .def_readonly("resabs", &Adapt2DResult::resabs)
      .def_readonly("tol", &Adapt2DResult::tol)
      .def_readonly("converged", &Adapt2DResult::converged)
      .def_readonly("evals", &Adapt2DResult::evals)
      .def_readonly("rounds", &Adapt2DResult::rounds)
      .def_readonly("intervals", &Adapt2DResult::intervals)
      .def_readonly("splits", &Adapt2DResult::splits)
      .def_readonly("splits_x", &Adapt2DResult::splits_x)
      .def_readonly("splits_y", &Adapt2DResult::splits_y)
      .def_readonly("floor", &Adapt2DResult::floor)
      .def_readonly("forced", &Adapt2DResult::forced)
      .def_readonly("nonfinite", &Adapt2DResult::nonfinite)
      .def_readonly("capped", &Adapt2DResult::capped)
      .def_readonly("device_ms", &Adapt2DResult::device_ms)
      .def("as_dict", [](const Adapt2DResult& r) {
        py::dict d;
        d["value"] = r.value;
        d["err_est"] = r.err_est;
        d["resabs"] = r.resabs;
        d["tol"] = r.tol;
        d["converged"] = r.converged;
        d["evals"] = r.evals;
        d["rounds"] = r.rounds;
        d["intervals"] = r.intervals;
        d["splits"] = r.splits;
        d["splits_x"] = r.splits_x;
        d["splits_y"] = r.splits_y;
        d["floor"] = r.floor;
        d["forced"] = r.forced;
        d["nonfinite"] = r.nonfinite;
        d["capped"] = r.capped;
        d["device_ms"] = r.device_ms;
        return d;
      });
  m.def("adapt2d_check", &adapt2d_check, py::arg("ax"), py::arg("bx"), py::arg("ay"),
        py::arg("by"), py::arg("options"),
        "raise, naming the numbers, unless the rectangle and the options are ones ExprAdaptive2D "
        "takes");
  m.def("expr_adapt2d_source", &expr_adapt2d_source, py::arg("expr"),
        "source of the adaptive 2-D kernels generated for an expression over x and y");
  m.def("expr_adapt2d_compile", compiled(&expr_adapt2d_compile), py::arg("expr"),
        "compile the adaptive 2-D kernels for gfx950 with hipRTC (no device needed)");
  py::class_<ExprAdaptive2D>(m, "ExprAdaptive2D",
                             "the integral of f(x, y) over a rectangle to a requested tolerance "
                             "(hipRTC, gfx950)")
      .def(py::init<const std::string&, int>(), py::arg("expr"), py::arg("device") = 0)
      .def("integrate",
           [](ExprAdaptive2D& e, double ax, double bx, double ay, double by,
              const Adapt2DOptions& o, uintptr_t out, uint64_t capacity) {
             return e.integrate(ax, bx, ay, by, o, reinterpret_cast<double*>(out), capacity);
           },
           py::arg("ax"), py::arg("bx"), py::arg("ay"), py::arg("by"),
           py::arg("options") = Adapt2DOptions(), py::arg("rects_out") = 0,
           py::arg("capacity") = 0, py::call_guard<py::gil_scoped_release>())
      .def("time", &ExprAdaptive2D::time, py::arg("ax"), py::arg("bx"), py::arg("ay"),
           py::arg("by"), py::arg("options"), py::arg("iters"),
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("expression", &ExprAdaptive2D::expression);

  // adaptive double integrals between two curves: y from ylo(x) to yhi(x)
  m.def("expr_region_source", &expr_region_source, py::arg("expr"), py::arg("ylo"),
        py::arg("yhi"),
        "source of the adaptive region kernels generated for f(x, y) and the two limits in y, "
        "expressions over x");
  m.def("expr_region_compile", compiled(&expr_region_compile), py::arg("expr"), py::arg("ylo"), py::arg("yhi"),
        "compile the adaptive region kernels for gfx950 with hipRTC (no device needed)");
  m.def("fma", py::vectorize([](double a, double b, double c) { return std::fma(a, b, c); }),
        py::arg("a"), py::arg("b"), py::arg("c"),
        "fma(a, b, c) element by element, rounded once: the y the region kernels form");
  py::class_<ExprAdaptiveRegion>(m, "ExprAdaptiveRegion",
                                 "the integral of f(x, y) for y between two curves ylo(x) and "
                                 "yhi(x) to a requested tolerance (hipRTC, gfx950)")
      .def(py::init<const std::string&, const std::string&, const std::string&, int>(),
           py::arg("expr"), py::arg("ylo"), py::arg("yhi"), py::arg("device") = 0)
      .def("integrate",
           [](ExprAdaptiveRegion& e, double ax, double bx, const Adapt2DOptions& o, uintptr_t out,
              uint64_t capacity) {
             return e.integrate(ax, bx, o, reinterpret_cast<double*>(out), capacity);
           },
           py::arg("ax"), py::arg("bx"), py::arg("options") = Adapt2DOptions(),
           py::arg("rects_out") = 0, py::arg("capacity") = 0,
           py::call_guard<py::gil_scoped_release>())
      .def("time", &ExprAdaptiveRegion::time, py::arg("ax"), py::arg("bx"), py::arg("options"),
           py::arg("iters"), py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("expression", &ExprAdaptiveRegion::expression)
      .def_property_readonly("y_lo", &ExprAdaptiveRegion::y_lo)
      .def_property_readonly("y_hi", &ExprAdaptiveRegion::y_hi);

  // adaptive sweeps: f(x, p0..p7) for K rows, each row to its own tolerance, in shared rounds
  m.attr("ADAPT_SWEEP_MAX_TOTAL_LIMIT") = kAdaptSweepMaxTotalLimit;
  m.attr("ADAPT_SWEEP_INITIAL_TOTAL") = kAdaptSweepInitialTotal;
  m.attr("ADAPT_SWEEP_MIN_PANELS") = kAdaptSweepMinPanels;
  py::class_<AdaptSweepOptions>(m, "AdaptSweepOptions",
                                "tolerances and bounds of an adaptive sweep (0: derived)")
      .def(py::init([](double rtol, double atol, uint64_t panels, int max_depth,
                       uint64_t max_intervals, uint64_t max_total, bool unbounded) {
             AdaptSweepOptions o;
             o.unbounded = unbounded;
             o.rtol = rtol;
             o.atol = atol;
             o.panels = panels;
             o.max_depth = max_depth;
             o.max_intervals = max_intervals;
             o.max_total = max_total;
             return o;
           }),
           py::arg("rtol") = 1e-10, py::arg("atol") = 0.0, py::arg("panels") = 0,
           py::arg("max_depth") = 60, py::arg("max_intervals") = 0,
           py::arg("max_total") = uint64_t(1) << 22, py::arg("unbounded") = false)
      .def_readwrite("unbounded", &AdaptSweepOptions::unbounded)
      .def_readwrite("rtol", &AdaptSweepOptions::rtol)
      .def_readwrite("atol", &AdaptSweepOptions::atol)
      .def_readwrite("panels", &AdaptSweepOptions::panels)
      .def_readwrite("max_depth", &AdaptSweepOptions::max_depth)
      .def_readwrite("max_intervals", &AdaptSweepOptions::max_intervals)
      .def_readwrite("max_total", &AdaptSweepOptions::max_total);
  {
    // per-row fields as numpy arrays (copies); the call's fields as numbers
    auto f64 = [](const std::vector<double>& v) {
      return py::array_t<double>(static_cast<py::ssize_t>(v.size()), v.data());
    };
    auto u64 = [](const std::vector<uint64_t>& v) {
      return py::array_t<uint64_t>(static_cast<py::ssize_t>(v.size()), v.data());
    };
    auto flag = [](const std::vector<uint8_t>& v) {
      py::array_t<bool> out(static_cast<py::ssize_t>(v.size()));
      for (size_t i = 0; i < v.size(); ++i) out.mutable_data()[i] = v[i] != 0;
      return out;
    };
    using R = AdaptSweepResult;
    py::class_<R>(m, "AdaptSweepResult",
                  "per-row arrays (value ... capped) and the call's rounds, evals, peak, device_ms")
        .def(py::init<>())
        .def_property_readonly("value", [f64](const R& r) { return f64(r.value); })
        .def_property_readonly("err_est", [f64](const R& r) { return f64(r.err_est); })
        .def_property_readonly("resabs", [f64](const R& r) { return f64(r.resabs); })
        .def_property_readonly("tol", [f64](const R& r) { return f64(r.tol); })
        .def_property_readonly("converged", [flag](const R& r) { return flag(r.converged); })
        .def_property_readonly("capped", [flag](const R& r) { return flag(r.capped); })
        .def_property_readonly("evals", [u64](const R& r) { return u64(r.evals); })
        .def_property_readonly("rounds", [u64](const R& r) { return u64(r.rounds); })
        .def_property_readonly("intervals", [u64](const R& r) { return u64(r.intervals); })
        .def_property_readonly("splits", [u64](const R& r) { return u64(r.splits); })
        .def_property_readonly("floor", [u64](const R& r) { return u64(r.floor); })
        .def_property_readonly("forced", [u64](const R& r) { return u64(r.forced); })
        .def_property_readonly("nonfinite", [u64](const R& r) { return u64(r.nonfinite); })
        .def_property_readonly("rows", &R::rows)
        .def_readonly("call_rounds", &R::call_rounds)
        .def_readonly("call_evals", &R::call_evals)
        .def_readonly("peak", &R::peak)
        .def_readonly("device_ms", &R::device_ms)
        .def_readonly("range", &R::range);
    using C = AdaptCurveResult;
    py::class_<C>(m, "AdaptCurveResult",
                  "per-point arrays (x, value, err_est, tol, resabs, converged; M + 1 entries), "
                  "the per-cell AdaptSweepResult `cells` and atol_cell, the totals and the call")
        .def(py::init<>())
        .def_property_readonly("x", [f64](const C& r) { return f64(r.x); })
        .def_property_readonly("value", [f64](const C& r) { return f64(r.value); })
        .def_property_readonly("err_est", [f64](const C& r) { return f64(r.err_est); })
        .def_property_readonly("tol", [f64](const C& r) { return f64(r.tol); })
        .def_property_readonly("resabs", [f64](const C& r) { return f64(r.resabs); })
        .def_property_readonly("converged", [flag](const C& r) { return flag(r.converged); })
        .def_property_readonly("atol_cell", [f64](const C& r) { return f64(r.atol_cell); })
        .def_readonly("cells", &C::cells)
        .def_property_readonly("points", &C::points)
        .def_readonly("total", &C::total)
        .def_readonly("total_err_est", &C::total_err_est)
        .def_readonly("total_tol", &C::total_tol)
        .def_readonly("total_resabs", &C::total_resabs)
        .def_readonly("unconverged", &C::unconverged)
        .def_readonly("call_rounds", &C::call_rounds)
        .def_readonly("call_evals", &C::call_evals)
        .def_readonly("peak", &C::peak)
        .def_readonly("device_ms", &C::device_ms);
    m.def("adapt_curve_atol",
          [f64](const std::vector<double>& x, double atol) {
            return f64(adapt_curve_atol(x, atol));
          },
          py::arg("x"), py::arg("atol"),
          "atol_c = (atol * |x[c + 1] - x[c]|) / |x[M] - x[0]| of every cell, in that order");
  }
  m.attr("ADAPT_CURVE_MAX_CELLS") = kAdaptCurveMaxCells;
  m.def("adapt_sweep_ranges_check", &adapt_sweep_ranges_check, py::arg("rows"),
        py::arg("nparams"), py::arg("param_count"), py::arg("a"), py::arg("b"),
        py::arg("options"),
        "adapt_sweep_check for per-row ranges a[r], b[r]; returns the resolved options");
  m.def("adapt_curve_check", &adapt_curve_check, py::arg("x"), py::arg("options"),
        "raise, naming the first offending index or the numbers, unless ExprAdaptiveCurve takes "
        "the grid; returns the options with a curve's panels and max_intervals resolved");
  m.def("expr_adapt_sweep_ranges_source", &expr_adapt_sweep_ranges_source,
        "source of the kernels that read per-row ranges and of the curve's prefix kernel");
  m.def("expr_adapt_sweep_ranges_compile", compiled(&expr_adapt_sweep_ranges_compile),
        "compile them for gfx950 with hipRTC (no device needed)");
  py::class_<ExprAdaptiveCurve>(m, "ExprAdaptiveCurve",
                                "F(x_j) = the integral of f from x_0 to x_j on a grid, every "
                                "cell to a tolerance (hipRTC, gfx950)")
      .def(py::init<const std::string&, int>(), py::arg("expr"), py::arg("device") = 0)
      .def("integrate", &ExprAdaptiveCurve::integrate, py::arg("x"),
           py::arg("options") = AdaptSweepOptions(), py::call_guard<py::gil_scoped_release>())
      .def("time_prefix", &ExprAdaptiveCurve::time_prefix, py::arg("cells"), py::arg("iters"),
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("expression", &ExprAdaptiveCurve::expression);
  m.def("expr_adapt_sweep_unbounded_source", &expr_adapt_sweep_unbounded_source, py::arg("expr"),
        py::arg("nparams"),
        "source of the sweep's eval kernels of the infinite kinds for f(x, p0..p{nparams-1})");
  m.def("expr_adapt_sweep_unbounded_compile", compiled(&expr_adapt_sweep_unbounded_compile),
        py::arg("expr"), py::arg("nparams"),
        "compile the sweep's unbounded eval kernels for gfx950 with hipRTC (no device needed)");
  m.def("adapt_sweep_default_panels", &adapt_sweep_default_panels, py::arg("rows"),
        "the panels a sweep of `rows` rows starts from unless told");
  m.def("adapt_sweep_check", &adapt_sweep_check, py::arg("rows"), py::arg("nparams"),
        py::arg("param_count"), py::arg("a"), py::arg("b"), py::arg("options"),
        "raise, naming the numbers, unless ExprAdaptiveSweep takes the call; returns the options "
        "with panels = 0 and max_intervals = 0 resolved");
  m.def("expr_adapt_sweep_source", &expr_adapt_sweep_source, py::arg("expr"), py::arg("nparams"),
        "source of the adaptive sweep kernels generated for f(x, p0..p{nparams-1})");
  m.def("expr_adapt_sweep_compile", compiled(&expr_adapt_sweep_compile), py::arg("expr"),
        py::arg("nparams"),
        "compile the adaptive sweep kernels for gfx950 with hipRTC (no device needed)");
  py::class_<ExprAdaptiveSweep>(m, "ExprAdaptiveSweep",
                                "f(x, p0..p7) for K rows, each to a requested tolerance (hipRTC)")
      .def(py::init<const std::string&, int, int>(), py::arg("expr"), py::arg("nparams"),
           py::arg("device") = 0)
      .def("integrate",
           [](ExprAdaptiveSweep& e, const ParamRows& params, double a, double b,
              const AdaptSweepOptions& o) {
             uint64_t rows = 0;
             const std::vector<double> p = param_rows(params, e.nparams(), &rows);
             py::gil_scoped_release nogil;
             return e.integrate(p, rows, a, b, o);
           },
           py::arg("params"), py::arg("a"), py::arg("b"),
           py::arg("options") = AdaptSweepOptions())
      .def("time",
           [](ExprAdaptiveSweep& e, const ParamRows& params, double a, double b,
              const AdaptSweepOptions& o, int iters) {
             uint64_t rows = 0;
             const std::vector<double> p = param_rows(params, e.nparams(), &rows);
             py::gil_scoped_release nogil;
             return e.time(p, rows, a, b, o, iters);
           },
           py::arg("params"), py::arg("a"), py::arg("b"), py::arg("options"), py::arg("iters"))
      .def("integrate_ranges",
           [](ExprAdaptiveSweep& e, const ParamRows& params, const std::vector<double>& a,
              const std::vector<double>& b, const AdaptSweepOptions& o) {
             uint64_t rows = 0;
             const std::vector<double> p = param_rows(params, e.nparams(), &rows);
             py::gil_scoped_release nogil;
             return e.integrate_ranges(p, rows, a, b, o);
           },
           py::arg("params"), py::arg("a"), py::arg("b"),
           py::arg("options") = AdaptSweepOptions(),
           "row r on its own [a[r], b[r]]: a and b hold one number per row")
      .def("time_ranges",
           [](ExprAdaptiveSweep& e, const ParamRows& params, const std::vector<double>& a,
              const std::vector<double>& b, const AdaptSweepOptions& o, int iters) {
             uint64_t rows = 0;
             const std::vector<double> p = param_rows(params, e.nparams(), &rows);
             py::gil_scoped_release nogil;
             return e.time_ranges(p, rows, a, b, o, iters);
           },
           py::arg("params"), py::arg("a"), py::arg("b"), py::arg("options"), py::arg("iters"))
      .def_property_readonly("expression", &ExprAdaptiveSweep::expression)
      .def_property_readonly("nparams", &ExprAdaptiveSweep::nparams);

  // integrals over a box in up to 16 variables: randomly shifted rank-1 lattice rules
  m.attr("LATTICE_MAX_DIM") = kLatticeMaxDim;
  m.attr("LATTICE_MIN_M") = kLatticeMinM;
  m.attr("LATTICE_MAX_M") = kLatticeMaxM;
  m.attr("LATTICE_MAX_SHIFTS") = kLatticeMaxShifts;
  m.attr("LATTICE_BUILTIN_M_MIN") = kLatticeBuiltinMin;
  m.attr("LATTICE_BUILTIN_M_MAX") = kLatticeBuiltinMax;
  m.def("lattice_generator", &lattice_generator, py::arg("m"), py::arg("d"),
        "the built-in Korobov vector z_j = a^j mod 2^m, j < d");
  m.def("lattice_multiplier", &lattice_multiplier, py::arg("m"),
        "the built-in table's Korobov multiplier a of m");
  m.def("lattice_shifts",
        [](uint64_t seed, int shifts, int d) {
          const std::vector<uint32_t> w = lattice_shifts(seed, shifts, d);
          py::array_t<uint32_t> a({static_cast<py::ssize_t>(shifts), static_cast<py::ssize_t>(d)});
          std::copy(w.begin(), w.end(), a.mutable_data());
          return a;
        },
        py::arg("seed"), py::arg("shifts"), py::arg("d"),
        "the shifts x d shift words of a seed: the high 32 bits of splitmix64 at r * 16 + j");
  py::class_<LatticeOptions>(m, "LatticeOptions", "shifts, generating vector and tolerances")
      .def(py::init([](int shifts, uint64_t seed, std::vector<uint32_t> shift_words,
                       std::vector<uint64_t> z, double rtol, double atol, int m_min, int m_max) {
             LatticeOptions o;
             o.shifts = shifts;
             o.seed = seed;
             o.shift_words = std::move(shift_words);
             o.z = std::move(z);
             o.rtol = rtol;
             o.atol = atol;
             o.m_min = m_min;
             o.m_max = m_max;
             return o;
           }),
           py::arg("shifts") = 16, py::arg("seed") = 0,
           py::arg("shift_words") = std::vector<uint32_t>(),
           py::arg("z") = std::vector<uint64_t>(), py::arg("rtol") = 0.0, py::arg("atol") = 0.0,
           py::arg("m_min") = 12, py::arg("m_max") = 0)
      .def_readwrite("shifts", &LatticeOptions::shifts)
      .def_readwrite("seed", &LatticeOptions::seed)
      .def_readwrite("shift_words", &LatticeOptions::shift_words)
      .def_readwrite("z", &LatticeOptions::z)
      .def_readwrite("rtol", &LatticeOptions::rtol)
      .def_readwrite("atol", &LatticeOptions::atol)
      .def_readwrite("m_min", &LatticeOptions::m_min)
      .def_readwrite("m_max", &LatticeOptions::m_max);
  py::class_<LatticeResult>(m, "LatticeResult", "value, error estimate and estimates of one call")
      .def_readonly("value", &LatticeResult::value)
      .def_readonly("err_est", &LatticeResult::err_est)
      .def_property_readonly("estimates",
                             [](const LatticeResult& r) {
                               return py::array_t<double>(
                                   static_cast<py::ssize_t>(r.estimates.size()),
                                   r.estimates.data());
                             })
      .def_readonly("m", &LatticeResult::m)
      .def_readonly("n", &LatticeResult::n)
      .def_readonly("shifts", &LatticeResult::shifts)
      .def_readonly("evals", &LatticeResult::evals)
      .def_readonly("levels", &LatticeResult::levels)
      .def_readonly("converged", &LatticeResult::converged)
      .def_readonly("device_ms", &LatticeResult::device_ms)
      .def("as_dict", [](const LatticeResult& r) {
        py::dict d;
        d["value"] = r.value;
        d["err_est"] = r.err_est;
        d["estimates"] = r.estimates;
        d["m"] = r.m;
        d["n"] = r.n;
        d["shifts"] = r.shifts;
        d["evals"] = r.evals;
        d["levels"] = r.levels;
        d["converged"] = r.converged;
        d["device_ms"] = r.device_ms;
        return d;
      });
  m.def("lattice_check", &lattice_check, py::arg("box"), py::arg("m"), py::arg("options"),
        py::arg("begin"), py::arg("count"), py::arg("scale") = 1.0,
        "raise, naming the numbers, unless ExprLattice.integrate takes the box, the level, the "
        "options and the slice");
  m.def("lattice_check_walk", &lattice_check_walk, py::arg("box"), py::arg("options"),
        py::arg("scale") = 1.0,
        "raise, naming the numbers, unless ExprLattice.integrate_to takes the box and the options");
  m.def("lattice_shape", [](uint64_t count, int shifts, int grid) {
          const LatticeShape s = lattice_shape(count, shifts, grid);
          return py::make_tuple(s.gx, s.gy);
        },
        py::arg("count"), py::arg("shifts"), py::arg("grid") = 0,
        "(gx, gy) of a lattice launch; gx never depends on shifts");
  m.def("expr_lattice_source", &expr_lattice_source, py::arg("expr"), py::arg("d"),
        py::arg("periodic") = false,
        "source of the lattice kernels generated for an expression over x0..x{d-1}");
  m.def("expr_lattice_compile", compiled(&expr_lattice_compile), py::arg("expr"), py::arg("d"),
        py::arg("periodic") = false,
        "compile the lattice kernels for gfx950 with hipRTC (no device needed)");
  py::class_<ExprLattice>(m, "ExprLattice",
                          "the integral of f(x0..x{d-1}) over a box by a randomly shifted rank-1 "
                          "lattice rule (hipRTC, gfx950)")
      .def(py::init<const std::string&, int, bool, int, int>(), py::arg("expr"), py::arg("d"),
           py::arg("periodic") = false, py::arg("device") = 0, py::arg("grid") = 0)
      .def("integrate",
           [](ExprLattice& e, const LatticeBox& box, int lm, const LatticeOptions& o,
              uint64_t begin, py::object count, double scale, const Comm* comm) {
             const uint64_t c = count.is_none() ? ~0ull : count.cast<uint64_t>();
             py::gil_scoped_release nogil;
             return e.integrate(box, lm, o, begin, c, scale, comm);
           },
           py::arg("box"), py::arg("m"), py::arg("options") = LatticeOptions(),
           py::arg("begin") = 0, py::arg("count") = py::none(), py::arg("scale") = 1.0,
           py::arg("comm") = nullptr)
      .def("integrate_to", &ExprLattice::integrate_to, py::arg("box"), py::arg("options"),
           py::arg("scale") = 1.0, py::arg("comm") = nullptr,
           py::call_guard<py::gil_scoped_release>())
      .def("time",
           [](ExprLattice& e, const LatticeBox& box, int lm, const LatticeOptions& o,
              uint64_t begin, py::object count, int iters) {
             const uint64_t c = count.is_none() ? ~0ull : count.cast<uint64_t>();
             py::gil_scoped_release nogil;
             return e.time(box, lm, o, begin, c, iters);
           },
           py::arg("box"), py::arg("m"), py::arg("options") = LatticeOptions(),
           py::arg("begin") = 0, py::arg("count") = py::none(), py::arg("iters") = 10)
      .def("use_partials",
           [](ExprLattice& e, uintptr_t ptr, uint64_t capacity) {
             e.use_partials(reinterpret_cast<double*>(ptr), capacity);
           },
           py::arg("device_ptr"), py::arg("capacity"),
           "partials go to the caller's device memory (capacity doubles); 0: the object's own")
      .def_property_readonly("expression", &ExprLattice::expression)
      .def_property_readonly("dim", &ExprLattice::dim)
      .def_property_readonly("periodic", &ExprLattice::periodic);

  // ------------------------------------------------------------------ host (CPU) engine
  m.def("host_isa", &host_isa, "vector ISA the host kernels dispatch to: avx512|avx2|base");
  py::class_<HostPool>(m, "HostPool", "persistent host worker threads (0 = one per core)")
      .def(py::init<int>(), py::arg("threads") = 0)
      .def_property_readonly("threads", &HostPool::threads)
      .def_static("default_threads", &HostPool::default_threads);
  m.def("host_riemann", &host_riemann, py::arg("config"), py::arg("begin"), py::arg("count"),
        py::arg("pool"), py::call_guard<py::gil_scoped_release>(),
        "h * scale * sum of f over samples [begin, begin + count), per-sample fp64 on threads");
  py::class_<HostExpr>(m, "HostExpr", "f(x) as an expression, compiled for the host cores")
      .def(py::init<const std::string&>(), py::arg("expr"),
           py::call_guard<py::gil_scoped_release>())
      .def("integrate", &HostExpr::integrate, py::arg("a"), py::arg("b"), py::arg("n"),
           py::arg("rule"), py::arg("begin"), py::arg("count"), py::arg("pool"),
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("expression", &HostExpr::expression);
  py::class_<HostExprSweep>(m, "HostExprSweep",
                            "f(x, p0..p7) as an expression, K rows on the host cores")
      .def(py::init<const std::string&, int>(), py::arg("expr"), py::arg("nparams"),
           py::call_guard<py::gil_scoped_release>())
      .def("integrate",
           [](const HostExprSweep& e, const ParamRows& params, double a, double b, uint64_t n,
              Rule rule, uint64_t begin, uint64_t count, HostPool& pool) {
             uint64_t rows = 0;
             const std::vector<double> p = param_rows(params, e.nparams(), &rows);
             std::vector<double> v;
             {
               py::gil_scoped_release nogil;
               v = e.integrate(p, rows, a, b, n, rule, begin, count, pool);
             }
             return py::array_t<double>(static_cast<py::ssize_t>(v.size()), v.data());
           },
           py::arg("params"), py::arg("a"), py::arg("b"), py::arg("n"), py::arg("rule"),
           py::arg("begin"), py::arg("count"), py::arg("pool"))
      .def_property_readonly("expression", &HostExprSweep::expression)
      .def_property_readonly("nparams", &HostExprSweep::nparams);
  py::class_<HostExpr2D>(m, "HostExpr2D", "f(x, y) as an expression, on the host cores")
      .def(py::init<const std::string&>(), py::arg("expr"),
           py::call_guard<py::gil_scoped_release>())
      .def("integrate", &HostExpr2D::integrate, py::arg("ax"), py::arg("bx"), py::arg("nx"),
           py::arg("ay"), py::arg("by"), py::arg("ny"), py::arg("rule"), py::arg("row_begin"),
           py::arg("row_count"), py::arg("pool"), py::arg("scale") = 1.0,
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("expression", &HostExpr2D::expression);
  m.def("host_riemann_mpi_parity", &host_riemann_mpi_parity, py::arg("comm_size"), py::arg("n"),
        py::arg("range"), py::arg("pool"), py::call_guard<py::gil_scoped_release>(),
        "the reference's mpirun -np P ./riemann, bit for bit, with its P-1 workers on threads");
  py::class_<HostComm>(m, "HostComm", "host collectives between processes (TCP star via rank 0)")
      .def(py::init<const std::string&, int, int, int, double>(), py::arg("addr"),
           py::arg("port"), py::arg("rank"), py::arg("world"), py::arg("timeout_s") = 120.0,
           py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("rank", &HostComm::rank)
      .def_property_readonly("world", &HostComm::world)
      .def("allreduce_sum", [](HostComm& c, std::vector<double> v) {
             py::gil_scoped_release nogil;
             c.allreduce_sum(v.data(), v.size());
             return v;
           })
      .def("allgather", [](HostComm& c, std::vector<double> v) {
             std::vector<double> out(v.size() * c.world());
             py::gil_scoped_release nogil;
             c.allgather(v.data(), out.data(), v.size());
             return out;
           })
      .def("broadcast", [](HostComm& c, std::vector<double> v, int root) {
             py::gil_scoped_release nogil;
             c.broadcast(v.data(), v.size(), root);
             return v;
           })
      .def("barrier", &HostComm::barrier, py::call_guard<py::gil_scoped_release>());
  m.def("host_trainscan", [](int sps, int seconds, HostPool& pool, HostComm* comm, bool keep,
                             std::vector<double> table) {
          HostScanConfig c;
          c.steps_per_sec = sps;
          c.seconds = seconds;
          c.keep = keep;
          c.table = std::move(table);
          std::vector<double> vel, pos;
          HostScanResult r;
          {
            py::gil_scoped_release nogil;
            r = host_trainscan(c, pool, comm, keep ? &vel : nullptr, keep ? &pos : nullptr);
          }
          py::dict d;
          d["distance"] = r.distance;
          d["sum_of_sums"] = r.sum_of_sums;
          d["seconds"] = r.seconds;
          d["begin"] = r.begin;
          d["count"] = r.count;
          if (keep) {
            d["velocity"] = vel;
            d["position"] = pos;
          }
          return d;
        },
        py::arg("steps_per_sec") = 10000, py::arg("seconds") = 1800, py::arg("pool"),
        py::arg("comm") = nullptr, py::arg("keep") = false,
        py::arg("table") = std::vector<double>{});

  // ------------------------------------------------------------------ oracle
  py::module_ o = m.def_submodule("oracle", "host oracles, generated fixtures, parity emulation");
  o.def("profile_table", &oracle::profile_table);
  o.def("generated_profile_table", &oracle::generated_profile_table);
  o.def("faccel_ref", [](double t) { return oracle::faccel_ref(oracle::profile_table(), t); });
  o.def("interp", [](double t) { return oracle::interp(oracle::profile_table(), t); });
  o.def("profile_exact_integral", &oracle::profile_exact_integral);
  o.def("load_profile", &oracle::load_profile, py::arg("path"),
        "a velocity profile (CSV/text numbers, 1 s spacing)");
  o.def("table_integral", &oracle::table_integral, py::arg("table"), py::arg("a"), py::arg("b"),
        "exact integral of the table's piecewise-linear interpolant over [a, b]");
  o.def("analytic", &oracle::analytic, py::arg("integrand"), py::arg("a"), py::arg("b"),
        py::arg("coef") = std::vector<double>{}, py::arg("p0") = 0.0, py::arg("p1") = 0.0);
  o.def("riemann_serial", [](Integrand f, double a, double b, uint64_t n, Rule r,
                             std::vector<double> coef, double p0, double p1) {
    py::gil_scoped_release nogil;
    return static_cast<double>(oracle::riemann_serial(f, a, b, n, r, coef, p0, p1));
  }, py::arg("integrand"), py::arg("a"), py::arg("b"), py::arg("n"), py::arg("rule"),
     py::arg("coef") = std::vector<double>{}, py::arg("p0") = 0.0, py::arg("p1") = 0.0);
  o.def("riemann_mpi_parity", &oracle::riemann_mpi_parity, py::arg("comm_size"), py::arg("n"),
        py::arg("range") = 3.14159265358979323846, py::call_guard<py::gil_scoped_release>());
  o.def("cintegrate_parity", &oracle::cintegrate_parity, py::call_guard<py::gil_scoped_release>());
  o.def("trainscan_parity", [](int p) {
    oracle::TrainScanParity r;
    {
      py::gil_scoped_release nogil;
      r = oracle::trainscan_parity(p);
    }
    return py::make_tuple(r.distance, r.sum_of_sums);
  });
  o.def("train_distance", &oracle::train_distance);
  o.attr("TRAIN_TS") = oracle::kTrainTs;
  o.attr("TRAIN_VS") = oracle::kTrainVs;
  o.attr("TRAIN_AS") = oracle::kTrainAs;
  o.attr("STEPS_PER_SEC") = oracle::kStepsPerSec;
  o.attr("PROFILE_SECONDS") = oracle::kProfileSeconds;
}
