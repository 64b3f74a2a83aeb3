// pf_graph.h — stream capture into an instantiated hipGraph: the one place the library begins a capture (pf_api.hip: the
// GD and sharded iteration graphs; pf_pcg.hip: the CG iteration graphs).  Host code only.
#pragma once
#include "pf_common.h"

struct pf_capture {
  hipStream_t s, a;   // the captured stream and the side branch (null when no events were asked for)
  hipEvent_t* ev;     // the `nev` events the enqueueing code joins its branches with
};

// capture fn(capture streams/events) on `s` and instantiate the graph; handle for pf_graph_launch / pf_graph_destroy.
// nev > 0: a side stream and nev events for the graph's branches; nev == 0 (a single chain): neither is created
template <class F>
static int capture_graph(hipStream_t s, int nev, hipStreamCaptureMode mode, void** graph_out, F&& fn) {
  auto fail = [](const char* msg) { pf_set_error(msg); return (int)PF_ERR_HIP; };
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipStream_t side = nullptr;
  hipEvent_t* ev = new hipEvent_t[nev];
  int made = 0;
  bool ok = nev == 0 || hipStreamCreateWithFlags(&side, hipStreamNonBlocking) == hipSuccess;
  for (; ok && made < nev; ++made)
    if (hipEventCreateWithFlags(&ev[made], hipEventDisableTiming) != hipSuccess) break;
  ok = ok && made == nev;
  auto cleanup = [&]() {
    for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]);
    delete[] ev;
    if (side) (void)hipStreamDestroy(side);
  };
  if (!ok) {
    cleanup();
    return fail("graph capture: stream/event creation failed");
  }
  if (hipStreamBeginCapture(s, mode) != hipSuccess) {
    cleanup();
    return fail("graph capture: the stream did not enter capture mode");
  }
  pf_capture cap{s, side, ev};
  const int rc = fn(cap);
  const hipError_t e = hipStreamEndCapture(s, &graph);
  cleanup();
  if (rc != PF_OK) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  if (e != hipSuccess || !graph) return fail("hipStreamEndCapture failed");
  if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGraphDestroy(graph);
    return fail("hipGraphInstantiate failed");
  }
  (void)hipGraphDestroy(graph);
  *graph_out = (void*)exec;
  return PF_OK;
}
