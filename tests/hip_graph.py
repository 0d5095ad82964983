"""Stream capture and graph replay for the tests: a ctypes binding to the HIP runtime
that is already loaded in the process (helpers only, no tests).

One runtime per process (raytracer_amd.lib()'s comment): torch's, when torch is there,
serves the library too.  hip() therefore calls raytracer_amd.lib() first and then opens
the libamdhip64 that the process has mapped, by its path, which gives the loaded copy's
handle and never a second runtime.

Capture is thread-local (hipStreamCaptureModeThreadLocal): only this thread's calls are
checked against the capture.  No environment variable is set here, and nothing here
builds a graph by hand: every graph is what one stream recorded, in order.
"""
import ctypes as C

import raytracer_amd as R

MODE_THREAD_LOCAL = 1  # hipStreamCaptureModeThreadLocal
KERNEL, MEMCPY, MEMSET = 0, 1, 2  # hipGraphNodeType
TYPE_NAMES = {0: "kernel", 1: "memcpy", 2: "memset", 3: "host", 4: "graph", 5: "empty", 6: "wait event",
              7: "event record"}

_hip = None


class HipError(RuntimeError):
    def __init__(self, call, code):
        super().__init__(f"{call} failed: hipError {code}")
        self.code = code


def hip():
    global _hip
    if _hip is None:
        R.lib()
        path = None
        with open("/proc/self/maps") as fh:
            for line in fh:
                if "libamdhip64" in line:
                    path = line.split(None, 5)[-1].strip()
                    break
        if path is None:
            raise RuntimeError("no HIP runtime is loaded in this process")
        L = C.CDLL(path)
        vp, vpp, szp = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
        for name, args in {
            "hipStreamBeginCapture": [vp, C.c_int],
            "hipStreamEndCapture": [vp, vpp],
            "hipGraphGetNodes": [vp, vpp, szp],
            "hipGraphGetRootNodes": [vp, vpp, szp],
            "hipGraphGetEdges": [vp, vpp, vpp, szp],
            "hipGraphNodeGetType": [vp, C.POINTER(C.c_int)],
            "hipGraphInstantiateWithFlags": [vpp, vp, C.c_ulonglong],
            "hipGraphLaunch": [vp, vp],
            "hipGraphExecDestroy": [vp],
            "hipGraphDestroy": [vp],
        }.items():
            f = getattr(L, name)
            f.restype, f.argtypes = C.c_int, args
        _hip = L
    return _hip


def _check(call, code):
    if code != 0:
        raise HipError(call, code)


def _handles(call, graph):
    """The list a hipGraphGet{Nodes,RootNodes} call returns (count first, then the handles)."""
    n = C.c_size_t(0)
    _check(call.__name__, call(graph, None, C.byref(n)))
    if n.value == 0:
        return []
    arr = (C.c_void_p * n.value)()
    _check(call.__name__, call(graph, arr, C.byref(n)))
    return [arr[i] for i in range(n.value)]


class Capture:
    """with Capture(stream_ptr) as cap: ... library calls on that stream ...

    The capture is ALWAYS ended on the way out, also after an exception in the body and
    when hipStreamEndCapture itself reports that the capture was invalidated (the stream
    is usable again either way; cap.end_error then holds the code, and a body that
    raised nothing gets a HipError).  Afterwards: nodes(), roots(), edges(), types(),
    chain(), launch().  close() destroys the executable graph and the graph; the tests
    call it (or use `with closing(...)`), and __del__ does as a last resort."""

    def __init__(self, stream_ptr):
        assert stream_ptr, "capture needs a stream of the caller's"
        self.stream = C.c_void_p(stream_ptr)
        self.graph = C.c_void_p(None)
        self.exe = C.c_void_p(None)
        self.end_error = 0

    def __enter__(self):
        _check("hipStreamBeginCapture", hip().hipStreamBeginCapture(self.stream, MODE_THREAD_LOCAL))
        return self

    def __exit__(self, etype, exc, tb):
        self.end_error = hip().hipStreamEndCapture(self.stream, C.byref(self.graph))
        if self.end_error != 0:
            if self.graph:
                hip().hipGraphDestroy(self.graph)
            self.graph = C.c_void_p(None)
            if etype is None:
                raise HipError("hipStreamEndCapture", self.end_error)
        elif etype is not None:
            self.close()
        return False

    # ---- the graph's shape
    def nodes(self):
        return _handles(hip().hipGraphGetNodes, self.graph)

    def roots(self):
        return _handles(hip().hipGraphGetRootNodes, self.graph)

    def edges(self):
        n = C.c_size_t(0)
        _check("hipGraphGetEdges", hip().hipGraphGetEdges(self.graph, None, None, C.byref(n)))
        if n.value == 0:
            return []
        a, b = (C.c_void_p * n.value)(), (C.c_void_p * n.value)()
        _check("hipGraphGetEdges", hip().hipGraphGetEdges(self.graph, a, b, C.byref(n)))
        return [(a[i], b[i]) for i in range(n.value)]

    def node_type(self, node):
        t = C.c_int(-1)
        _check("hipGraphNodeGetType", hip().hipGraphNodeGetType(C.c_void_p(node), C.byref(t)))
        return t.value

    def chain(self):
        """The node types in execution order, for a graph that is one chain; asserts that
        it is one: one root, nodes - 1 edges, no node with two successors or predecessors."""
        nodes, roots, edges = self.nodes(), self.roots(), self.edges()
        if not nodes:
            return []
        assert len(roots) == 1, f"{len(roots)} root nodes"
        assert len(edges) == len(nodes) - 1, f"{len(nodes)} nodes, {len(edges)} edges"
        succ = {}
        for a, b in edges:
            assert a not in succ, "a node with two successors: the graph has parallel branches"
            succ[a] = b
        assert len({b for _, b in edges}) == len(edges), "a node with two predecessors"
        order, at = [], roots[0]
        while at is not None:
            order.append(at)
            at = succ.get(at)
        assert len(order) == len(nodes), "the graph is not one chain"
        return [self.node_type(n) for n in order]

    # ---- replay
    def launch(self, stream_ptr=None):
        """One replay, enqueued on stream_ptr (default: the stream that captured)."""
        assert self.graph, "no graph (the capture failed)"
        if not self.exe:
            _check("hipGraphInstantiateWithFlags",
                   hip().hipGraphInstantiateWithFlags(C.byref(self.exe), self.graph, 0))
        s = C.c_void_p(stream_ptr) if stream_ptr else self.stream
        _check("hipGraphLaunch", hip().hipGraphLaunch(self.exe, s))

    def close(self):
        """Destroys what the capture made (the device must be done with the last replay)."""
        if self.exe:
            hip().hipGraphExecDestroy(self.exe)
            self.exe = C.c_void_p(None)
        if self.graph:
            hip().hipGraphDestroy(self.graph)
            self.graph = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
