// A batch of launches with fixed arguments, captured once into a hipGraph and replayed (the five iteration loops of the
// library are launch-bound on small problems).  Direct launches stay each loop's fallback when a batch is not ready().
#pragma once

#include <cstdlib>

#include "sx_internal.h"

struct SxGraphBatch {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    SxGraphBatch() = default;
    SxGraphBatch(const SxGraphBatch &) = delete;
    SxGraphBatch &operator=(const SxGraphBatch &) = delete;
    ~SxGraphBatch() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
    // capture what `enqueue` launches on s (thread-local mode) and instantiate it.  On any failure the batch stays
    // not ready and the runtime's sticky error is cleared: the caller goes on with direct launches.
    template <class F>
    bool capture(hipStream_t s, F &&enqueue) {
        bool ok = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            enqueue();
            ok = hipStreamEndCapture(s, &graph) == hipSuccess && graph != nullptr &&
                 hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
        }
        if (!ok) {
            exec = nullptr;
            (void)hipGetLastError();
        }
        return ok;
    }
    bool ready() const { return exec != nullptr; }
    hipError_t launch(hipStream_t s) { return hipGraphLaunch(exec, s); }
};

// When a loop replays, besides its own size rule: option "graph" (ctx->opt_graph) switches all five off, and each loop
// heeds the environment as it always has --
//
//   loop                                  SX_NO_GRAPH set    under a profiler (ROCP_TOOL_LIBRARIES set)
//   first-order LP stage (sx_pdlp.hip)    direct launches    direct launches, unless SX_GRAPH_UNDER_PROFILER is set
//   dense simplex (sx_simplex.hip)        ignored            direct launches
//   CG (sx_cg.hip)                        direct launches    ignored
//   Sinkhorn, single and batched          ignored            ignored
//
// SX_NO_GRAPH asks for direct launches (readable traces).  rocprofv3 --kernel-trace (ROCm 7.2) faults inside
// hipGraphLaunch after some thousands of replays: profiles/r03/hipgraph_rocprofv3.md, the frames are named in
// profiles/r04/hipgraph_frames.md; SX_GRAPH_UNDER_PROFILER=1 keeps the graph path there -- to reproduce the fault, not
// to measure.  The rows differ because each loop got its rule when it needed one; making them one rule changes
// behaviour and is a decision of its own.
constexpr unsigned SX_GRAPH_HEED_NO_GRAPH_ENV = 1u;
constexpr unsigned SX_GRAPH_HEED_PROFILER = 2u;
constexpr unsigned SX_GRAPH_HEED_PROFILER_OVERRIDE = 4u; // with HEED_PROFILER: SX_GRAPH_UNDER_PROFILER lifts it
inline bool sx_graph_wanted(const sx_ctx *ctx, unsigned heed) {
    if (!ctx->opt_graph) return false;
    if ((heed & SX_GRAPH_HEED_NO_GRAPH_ENV) && getenv("SX_NO_GRAPH") != nullptr) return false;
    if ((heed & SX_GRAPH_HEED_PROFILER) && getenv("ROCP_TOOL_LIBRARIES") != nullptr)
        return (heed & SX_GRAPH_HEED_PROFILER_OVERRIDE) && getenv("SX_GRAPH_UNDER_PROFILER") != nullptr;
    return true;
}
