"""Host-side mirror of the reference's factor-graph surface (R/factor_net.R, R/factor_methods.R): W(), H(), factor_config(),
factor_input(), nmf_layer(), svd_layer(), factor_shared(), factor_concat(), factor_add(), factor_condition(), factor_net(), fit(),
predict().  R's `x |> nmf_layer(k = 8)` is `nmf_layer(x, k=8)` here.

Execution paths of fit():
  one nmf_layer on an input          the existing nmf() with the graph's config and seed, sort_model=True (graph/fit.hpp:213-242
                                     fit_single_layer; W_0 from R's runif as R/factor_methods.R:1005-1009)
  one nmf_layer on factor_shared()   the inputs row-stacked (all sparse: as one CSC, rows offset in argument order,
                                     graph/builder.hpp:438-457; otherwise densely), the same nmf() call, W split by the inputs' row
                                     counts into a dict keyed by input name ("input<i>" for an unnamed one), in ARGUMENT order (the
                                     R-level path; the compiled path splits in std::map order, RcppFunctions_graph.cpp:336-341)
  more than one layer                rcppml_gpu_factor_net_fit_ex (csrc/ops_graph.hip): the reference's fit_deep (graph/fit.hpp:264-375)
                                     resident on the device, fp64, loss = "mse"
Anything the backend does not implement raises NotImplementedError naming the option; nothing falls back to something else.
"""
import numpy as np

from . import _abi
from . import nmf as _nmf
from .data import CSC

_LOSSES = ("mse", "gp", "nb", "gamma", "inverse_gaussian", "tweedie")
_IRLS_LOSSES = _LOSSES[1:]
_NORMS = ("L1", "L2", "none")
_SOLVERS = ("auto", "cholesky", "cd")
_SVD_METHODS = ("auto", "deflation", "krylov", "lanczos", "irlba", "randomized")
_FIELDS = ("L1", "L2", "L21", "angular", "upper_bound")
MAX_DEEP_RANK = 128


def _match_arg(value, choices):
    if value not in choices:
        raise ValueError("'arg' should be one of %s" % ", ".join("'%s'" % c for c in choices))          # match.arg
    return value


# ------------------------------------------------------------------------------------------------------- per-factor configs
class FactorConfig:
    """fn_factor_config (R/factor_net.R:60-72): a field left at None inherits the layer's default."""

    def __init__(self, side, L1, L2, L21, angular, upper_bound, nonneg, graph, graph_lambda, target, target_lambda):
        if target is not None and np.ndim(target) != 2:
            raise ValueError("'target' must be a numeric matrix or NULL")                               # :63-64
        self.side = side
        self.L1, self.L2, self.L21, self.angular, self.upper_bound, self.nonneg = L1, L2, L21, angular, upper_bound, nonneg
        self.graph, self.graph_lambda, self.target, self.target_lambda = graph, graph_lambda, target, target_lambda

    def __repr__(self):
        return "fn_factor_config: %s-side" % self.side


def W(L1=None, L2=None, L21=None, angular=None, upper_bound=None, nonneg=None, graph=None, graph_lambda=None, target=None,
      target_lambda=None):
    """Per-factor settings of the W side (R/factor_net.R:42-48)."""
    return FactorConfig("W", L1, L2, L21, angular, upper_bound, nonneg, graph, graph_lambda, target, target_lambda)


def H(L1=None, L2=None, L21=None, angular=None, upper_bound=None, nonneg=None, graph=None, graph_lambda=None, target=None,
      target_lambda=None):
    """Per-factor settings of the H side (R/factor_net.R:52-58)."""
    return FactorConfig("H", L1, L2, L21, angular, upper_bound, nonneg, graph, graph_lambda, target, target_lambda)


class GlobalConfig:
    """fn_global_config (R/factor_net.R:126-157)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def factor_config(maxit=100, tol=1e-4, loss="mse", verbose=False, seed=None, threads=0, norm="L1", solver="auto", resource="auto",
                  test_fraction=0, cv_seed=0, mask_zeros=False, patience=5, precision=None, **dots):
    """R/factor_net.R:126-157.  `precision` (not in R): None = nmf()'s default for a single layer and fp64 for a deep graph; "fp64";
    "fp32" (single layer only).  `dots` are forwarded to nmf() on the single-layer paths as lowest-priority defaults."""
    _match_arg(loss, _LOSSES)
    _match_arg(norm, _NORMS)
    _match_arg(solver, _SOLVERS)
    if not (0 <= test_fraction < 1):
        raise ValueError("test_fraction >= 0 && test_fraction < 1 is not TRUE")                          # stopifnot, :140
    if precision not in (None, "fp32", "fp64"):
        raise ValueError("precision must be None, 'fp32' or 'fp64'")
    return GlobalConfig(maxit=int(maxit), tol=float(tol), loss=loss, verbose=verbose, seed=seed, threads=int(threads), norm=norm,
                        solver=solver, resource=resource, test_fraction=float(test_fraction), cv_seed=int(cv_seed),
                        mask_zeros=bool(mask_zeros), patience=int(patience), precision=precision, dots=dict(dots))


# --------------------------------------------------------------------------------------------------------------- graph nodes
class Node:
    """fn_node: type is one of input, nmf_layer, svd_layer, shared, concat, add, condition."""

    def __init__(self, type, **kw):
        self.type = type
        self.name = None
        self.__dict__.update(kw)

    def __repr__(self):
        s = "fn_node: %s" % self.type
        if self.name is not None:
            s += " (%s)" % self.name
        if getattr(self, "k", None) is not None:
            s += ", k=%d" % self.k
        return s


def _is_matrix(data):
    return isinstance(data, CSC) or hasattr(data, "tocsc") or (isinstance(data, np.ndarray) and data.ndim == 2)


def factor_input(data, name=None):
    """R/factor_net.R:179-194.  data: a dense 2-D array, a scipy sparse matrix or a CSC.  An unnamed input stays unnamed (R names it
    after the expression that produced it, which Python cannot see); multi-modal results call it "input<i>"."""
    if isinstance(data, (str, bytes)):
        raise NotImplementedError(".spz path inputs are not implemented by the MI355X backend (read the file with the .spz reader first)")
    if not _is_matrix(data):
        raise ValueError("'data' must be a dense matrix, dgCMatrix, or path to .spz file")               # :181-182
    if data.shape[0] == 0 or data.shape[1] == 0:
        raise ValueError("Input matrix cannot be empty (0 rows or 0 columns)")                           # :183-184
    return Node("input", data=data, name=name)


def _layer(kind, input, k, L1, L2, L21, angular, upper_bound, W, H, name, extra, dots):
    return Node(kind, input=input, k=int(k), layer_defaults=dict(L1=L1, L2=L2, L21=L21, angular=angular, upper_bound=upper_bound),
                W_config=W, H_config=H, name=name, dots=dict(dots), **extra)


def nmf_layer(input, k, L1=0, L2=0, L21=0, angular=0, upper_bound=0, mask=None, zi="none", projective=False, symmetric=False,
              robust=False, W=None, H=None, name=None, **dots):
    """R/factor_net.R:246-276."""
    if not isinstance(input, Node):
        raise ValueError("'input' must be an fn_node (from factor_input, nmf_layer, etc.)")             # :253-254
    if W is not None and not isinstance(W, FactorConfig):
        raise ValueError("'W' must be created by W()")                                                   # :255-256
    if H is not None and not isinstance(H, FactorConfig):
        raise ValueError("'H' must be created by H()")                                                   # :257-258
    _match_arg(zi, ("none", "row", "col"))
    return _layer("nmf_layer", input, k, L1, L2, L21, angular, upper_bound, W, H, name,
                  dict(mask=mask, zi=zi, projective=projective, symmetric=symmetric, robust=robust), dots)


def svd_layer(input, k, L1=0, L2=0, L21=0, angular=0, upper_bound=0, center=False, scale=False, method="auto", mask=None,
              robust=False, W=None, H=None, name=None, **dots):
    """R/factor_net.R:320-346.  Inside a deep graph this is the unconstrained layer the reference's compiled path makes of it."""
    if not isinstance(input, Node):
        raise ValueError("'input' must be an fn_node")                                                   # :327-328
    _match_arg(method, _SVD_METHODS)
    return _layer("svd_layer", input, k, L1, L2, L21, angular, upper_bound, W, H, name,
                  dict(center=center, scale=scale, method=method, mask=mask, robust=robust, zi="none", projective=False,
                       symmetric=False), dots)


def _merge(kind, inputs):
    if len(inputs) < 2:
        raise ValueError("factor_%s() requires at least 2 inputs" % kind)                               # :374-375, :407-408, :434-435
    if not all(isinstance(x, Node) for x in inputs):
        raise ValueError("All arguments to factor_%s() must be fn_node objects" % kind)                 # :376-377, :409-410, :436-437
    return list(inputs)


def factor_shared(*inputs):
    """R/factor_net.R:372-387: one H shared by several inputs, each with its own W."""
    inputs = _merge("shared", inputs)
    return Node("shared", inputs=inputs, input_names=[x.name if x.name is not None else "" for x in inputs])


def factor_concat(*inputs):
    """R/factor_net.R:405-415: the branches' H row-bound, k_out = k_1 + k_2 + ..."""
    return Node("concat", inputs=_merge("concat", inputs))


def factor_add(*inputs):
    """R/factor_net.R:432-450: the branches' H added elementwise; equal ranks."""
    inputs = _merge("add", inputs)
    ranks = [x.k for x in inputs if getattr(x, "k", None) is not None]
    if len(ranks) >= 2 and len(set(ranks)) > 1:
        raise ValueError("factor_add() requires all branches to have the same rank k, got: " + ", ".join(str(r) for r in ranks))   # :443-445
    return Node("add", inputs=inputs)


def factor_condition(input, Z):
    """R/factor_net.R:471-482: append the metadata Z (n x p or p x n) to the upstream H."""
    if not isinstance(input, Node):
        raise ValueError("'input' must be an fn_node")                                                   # :472-473
    try:
        Zm = np.asarray(Z, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("'Z' must be a numeric matrix")                                                 # :474-475
    if Zm.ndim == 1:
        Zm = Zm[:, None]                                                                                 # as.matrix of a vector: n x 1
    if Zm.ndim != 2:
        raise ValueError("'Z' must be a numeric matrix")
    return Node("condition", input=input, Z=Zm)


# ---------------------------------------------------------------------------------------------------------------- compilation
def _collect_layers(node, seen):
    """.fn_collect_layers (R/factor_net.R:551-565): post-order, input before layer, branches in argument order.  A layer reached
    through two branches is listed once."""
    if node.type in ("nmf_layer", "svd_layer"):
        out = _collect_layers(node.input, seen)
        if id(node) not in seen:
            seen.add(id(node))
            out.append(node)
        return out
    if node.type in ("shared", "concat", "add"):
        out = []
        for x in node.inputs:
            out += _collect_layers(x, seen)
        return out
    if node.type == "condition":
        return _collect_layers(node.input, seen)
    return []


def _collect_inputs(node, seen):
    if node.type == "input":
        if id(node) in seen:
            return []
        seen.add(id(node))
        return [node]
    if node.type in ("shared", "concat", "add"):
        out = []
        for x in node.inputs:
            out += _collect_inputs(x, seen)
        return out
    return _collect_inputs(node.input, seen)


class FactorNet:
    """factor_net (R/factor_net.R:536-543)."""

    def __init__(self, inputs, output, config, layers, input_nodes, names):
        self.inputs, self.output, self.config, self.layers, self.input_nodes = inputs, output, config, layers, input_nodes
        self.layer_names = names
        self.n_layers = len(layers)

    def __repr__(self):
        return "<factor_net: %d layer(s): %s>" % (self.n_layers, ", ".join(self.layer_names))


def factor_net(inputs, output, config=None):
    """R/factor_net.R:508-544: validate the topology and name the layers L1 .. Ln in topological order."""
    if config is None:
        config = factor_config()
    if isinstance(inputs, Node):
        inputs = [inputs]
    inputs = list(inputs)
    if not all(isinstance(x, Node) for x in inputs):
        raise ValueError("'inputs' must be fn_node objects")                                             # :512-513
    if not isinstance(output, Node):
        raise ValueError("'output' must be an fn_node")                                                  # :514-515
    if not isinstance(config, GlobalConfig):
        raise ValueError("'config' must be from factor_config()")                                        # :516-517
    layers = _collect_layers(output, set())
    input_nodes = _collect_inputs(output, set())
    in_graph = set(id(x) for x in input_nodes)
    graph_names = set(x.name for x in input_nodes if x.name is not None)
    missing = [str(x.name) for x in inputs if not (id(x) in in_graph or (x.name is not None and x.name in graph_names))]
    if missing:
        raise ValueError("Declared inputs not found in graph: " + ", ".join(missing))                    # :526-528
    names = [l.name if l.name is not None else "L%d" % (i + 1) for i, l in enumerate(layers)]           # :531-534
    return FactorNet(inputs, output, config, layers, input_nodes, names)


# -------------------------------------------------------------------------------------------------------------------- results
class LayerResult:
    def __init__(self, W, d, H, iterations, loss, converged):
        self.W, self.d, self.H, self.iterations, self.loss, self.converged = W, d, H, iterations, loss, converged

    def __repr__(self):
        return "<layer: k=%d, iterations=%s, loss=%.6g>" % (len(self.d), self.iterations, self.loss)


class FactorNetResult:
    """factor_net_result: layers by name (res["L1"], res.L1), n_layers, multi_modal, input_names, total_iterations, total_loss,
    converged; layer_losses for a deep fit."""

    def __init__(self, layers, config, multi_modal, input_names, total_iterations, total_loss, converged, layer_losses=None, misc=None):
        self.layers, self.config, self.n_layers = layers, config, len(layers)
        self.multi_modal, self.input_names = multi_modal, input_names
        self.total_iterations, self.total_loss, self.converged = total_iterations, total_loss, converged
        self.layer_losses, self.misc = layer_losses, misc or {}

    def __getitem__(self, name):
        return self.layers[name]

    def __getattr__(self, name):
        layers = self.__dict__.get("layers", {})
        if name in layers:
            return layers[name]
        raise AttributeError(name)

    def __repr__(self):
        return "<factor_net_result: %d layer(s), iterations=%s, loss=%.6g, converged=%s>" % (
            self.n_layers, self.total_iterations, self.total_loss, self.converged)


# -------------------------------------------------------------------------------------------------------------- descriptors
def solver_mode(config):
    """.fn_build_descriptor's rule (R/factor_methods.R:867-873): 0 = CD, 1 = Cholesky; auto is Cholesky for MSE."""
    if config.solver == "cd":
        return 0
    if config.solver == "cholesky":
        return 1
    return 0 if config.loss in _IRLS_LOSSES else 1


def factor_settings(layer):
    """The layer's resolved (W, H) settings (R/factor_methods.R:930-956): a W() / H() field wins over the layer default; nonneg
    defaults to True for nmf_layer and False for svd_layer."""
    ld, default_nn = layer.layer_defaults, layer.type == "nmf_layer"
    out = []
    for fc in (layer.W_config, layer.H_config):
        s = {f: (getattr(fc, f) if fc is not None and getattr(fc, f) is not None else ld[f]) for f in _FIELDS}
        s["nonneg"] = bool(fc.nonneg) if fc is not None and fc.nonneg is not None else default_nn
        s["graph_lambda"] = fc.graph_lambda if fc is not None and fc.graph_lambda is not None else 0
        s["graph"] = fc.graph if fc is not None else None
        s["target"] = fc.target if fc is not None else None
        s["target_lambda"] = fc.target_lambda if fc is not None and fc.target_lambda is not None else 0
        out.append(s)
    return out[0], out[1]


def orient_Z(Z, n):
    """graph/fit.hpp:177-190: Z with n columns is p x n; otherwise Z with n rows is transposed; otherwise an error."""
    if Z.shape[1] == n:
        return Z
    if Z.shape[0] == n:
        return Z.T
    raise ValueError("Conditioning Z dimension mismatch")


def _refuse_layer_options(net):
    for layer, name in zip(net.layers, net.layer_names):
        if layer.mask is not None:
            raise NotImplementedError("layer %s: mask is not implemented for factor graphs by the MI355X backend" % name)
        if layer.zi != "none":
            raise NotImplementedError("layer %s: zi is not implemented for factor graphs by the MI355X backend" % name)
        if layer.projective:
            raise NotImplementedError("layer %s: projective is not implemented for factor graphs by the MI355X backend" % name)
        if layer.symmetric:
            raise NotImplementedError("layer %s: symmetric is not implemented for factor graphs by the MI355X backend" % name)
        if not (layer.robust is False or layer.robust is None):
            raise NotImplementedError("layer %s: robust is not implemented for factor graphs by the MI355X backend" % name)


def _source(node):
    """(source node, Z or None) of a layer's input: conditions are walked through, the last one met wins (fit.hpp:118-125)."""
    Z = None
    while node.type == "condition":
        Z = node.Z
        node = node.input
    return node, Z


def deep_descriptor(net):
    """The flat description rcppml_gpu_factor_net_fit_ex takes, after the refusals of a multi-layer graph:
    dict(data, rank, src_kind, branches, cond_Z, L1, L2, upper_bound, nonneg) with per-layer (W, H) pairs."""
    cfg = net.config
    if cfg.loss != "mse":
        raise NotImplementedError("loss = '%s' in a multi-layer graph is not implemented by the MI355X backend (mse only)" % cfg.loss)
    if cfg.test_fraction > 0:
        raise NotImplementedError("test_fraction > 0 in a multi-layer graph is not implemented by the MI355X backend")
    if cfg.precision == "fp32":
        raise NotImplementedError("precision = 'fp32' in a multi-layer graph is not implemented by the MI355X backend (fp64 only)")
    index = {id(l): i for i, l in enumerate(net.layers)}
    rank, kind, branches, Zs, pens, nn = [], [], [], [], {"L1": [], "L2": [], "upper_bound": []}, []
    data = None
    for i, (layer, name) in enumerate(zip(net.layers, net.layer_names)):
        src, Z = _source(layer.input)
        if src.type == "shared":
            # the reference's own message (R/factor_methods.R:248-249)
            raise NotImplementedError("Deep NMF with factor_shared() requires single-layer; use factor_shared() only on the first layer, "
                                      "or restructure the graph")
        w, h = factor_settings(layer)
        for term in ("L21", "angular"):
            if w[term] != 0 or h[term] != 0:
                raise NotImplementedError("layer %s: %s in a multi-layer graph is not implemented by the MI355X backend" % (name, term))
        if w["graph"] is not None or h["graph"] is not None or w["graph_lambda"] != 0 or h["graph_lambda"] != 0:
            raise NotImplementedError("layer %s: graph regularisation in a multi-layer graph is not implemented by the MI355X backend" % name)
        if w["target"] is not None or h["target"] is not None or w["target_lambda"] != 0 or h["target_lambda"] != 0:
            raise NotImplementedError("layer %s: target regularisation in a multi-layer graph is not implemented by the MI355X backend" % name)
        if layer.k > MAX_DEEP_RANK:
            raise NotImplementedError("layer %s: a rank above %d in a multi-layer graph is not implemented by the MI355X backend" % (name, MAX_DEEP_RANK))
        if layer.k < 1:
            raise ValueError("k must be a positive integer")
        if src.type == "input":
            if Z is not None:
                raise NotImplementedError("layer %s: factor_condition() on an input is not implemented by the MI355X backend" % name)
            if data is not None and src.data is not data:
                raise NotImplementedError("a multi-layer graph over more than one input matrix is not implemented by the MI355X backend")
            data = src.data
            kind.append(_abi.GRAPH_SRC["input"])
            branches.append([])
        elif src.type in ("concat", "add"):
            br = []
            for b in src.inputs:
                if id(b) not in index:
                    raise ValueError("%s: branch layer not found" % src.type)                            # fit.hpp:139-140, :155-156
                br.append(index[id(b)])
            if len(br) > 8:
                raise NotImplementedError("more than 8 branches into factor_%s() are not implemented by the MI355X backend" % src.type)
            kind.append(_abi.GRAPH_SRC[src.type])
            branches.append(br)
        else:
            kind.append(_abi.GRAPH_SRC["layer"])
            branches.append([index[id(src)]])
        rank.append(layer.k)
        Zs.append(Z)
        for f in pens:
            pens[f].append((float(w[f]), float(h[f])))
        nn.append((w["nonneg"], h["nonneg"]))
    if data is None:
        raise ValueError("effective_input: cannot resolve input for first layer")                        # fit.hpp:169-170
    from .data import as_matrix
    csc, dense = as_matrix(data)
    m, n = (csc.shape if csc is not None else dense.shape)
    # a condition block is oriented against the rows of its layer's input, which depend on the upstream blocks: layer by layer
    Zo = []
    for i, Z in enumerate(Zs):
        p_sofar = [0 if q is None else q.shape[0] for q in Zo] + [0] * (len(rank) - len(Zo))
        rows = _abi.factor_net_dims(m, n, rank, kind, branches, p_sofar)[i][0]
        Zo.append(None if Z is None else np.ascontiguousarray(orient_Z(Z, rows)))
    return dict(csc=csc, dense=dense, m=m, n=n, rank=rank, src_kind=kind, branches=branches, cond_Z=Zo, L1=pens["L1"], L2=pens["L2"],
                upper_bound=pens["upper_bound"], nonneg=nn)


# ------------------------------------------------------------------------------------------------------------------------ fit
def _nmf_args(layer, config):
    """.fn_build_nmf_args (R/factor_methods.R:493-603) for the existing nmf()."""
    w, h = factor_settings(layer)
    if w["target"] is not None or w["target_lambda"] != 0:
        raise NotImplementedError("a target on W is not implemented by the MI355X backend")
    args = dict(k=layer.k, tol=config.tol, maxit=config.maxit, loss=config.loss, norm=config.norm, sort_model=True,
                solver="cd" if solver_mode(config) == 0 else "cholesky", resource="gpu")
    if config.resource not in ("auto", "gpu"):
        raise ValueError("rcppml_amd has no CPU path; resource must be 'auto' or 'gpu'")
    if config.seed is not None:
        args["seed"] = config.seed
    if config.precision is not None:
        args["precision"] = config.precision
    if config.test_fraction > 0:
        args["test_fraction"] = config.test_fraction
        args["patience"] = config.patience
        if config.mask_zeros:
            args["mask"] = "zeros"
    if config.cv_seed != 0:
        args["cv_seed"] = config.cv_seed
    for f in _FIELDS:
        args[f] = (w[f], h[f])
    args["nonneg"] = (w["nonneg"], h["nonneg"])
    if w["graph"] is not None:
        args["graph_W"] = w["graph"]
    if h["graph"] is not None:
        args["graph_H"] = h["graph"]
    args["graph_lambda"] = (w["graph_lambda"] if w["graph"] is not None else 0, h["graph_lambda"] if h["graph"] is not None else 0)
    if h["target"] is not None:
        args["target_H"] = h["target"]
        args["target_lambda"] = h["target_lambda"]
    extra = dict(config.dots)
    extra.update(layer.dots)
    for key, v in extra.items():
        args.setdefault(key, v)
    return args


def stack_shared(inputs):
    """The row-stack of factor_shared()'s inputs: (matrix, row counts).  All sparse: one CSC with the rows offset in argument order
    (graph/builder.hpp:438-457); otherwise a dense array."""
    mats = [x.data for x in inputs]
    ncols = set(int(a.shape[1]) for a in mats)
    if len(ncols) != 1:
        raise ValueError("All inputs to factor_shared() must have the same number of columns")           # R/factor_methods.R:164-165
    rows = [int(a.shape[0]) for a in mats]
    if all(isinstance(a, CSC) or hasattr(a, "tocsc") for a in mats):
        cs = [a if isinstance(a, CSC) else CSC.from_scipy(a) for a in mats]
        n = ncols.pop()
        counts = sum(np.diff(c.p).astype(np.int64) for c in cs)
        p = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        ii = np.empty(int(p[-1]), np.int32)
        xx = np.empty(int(p[-1]), np.float64)
        at = p[:-1].astype(np.int64).copy()
        off = 0
        for c, r in zip(cs, rows):
            lens = np.diff(c.p).astype(np.int64)
            col = np.repeat(np.arange(n), lens)
            dst = at[col] + (np.arange(int(c.p[-1])) - np.repeat(c.p[:-1].astype(np.int64), lens))
            ii[dst] = np.asarray(c.i, np.int32) + off
            xx[dst] = c.x
            at += lens
            off += r
        return CSC((off, n), p, ii, xx), rows
    dense = [a.to_scipy().toarray() if isinstance(a, CSC) else (a.toarray() if hasattr(a, "tocsc") else np.asarray(a, np.float64)) for a in mats]
    return np.vstack(dense), rows


def _fit_single(net):
    layer, name = net.layers[0], net.layer_names[0]
    src, Z = _source(layer.input)
    if layer.type == "svd_layer":
        raise NotImplementedError("a single svd_layer is not implemented by the MI355X backend: the reference's compiled path runs an "
                                  "unconstrained ALS there, not svd(); call svd() directly")
    if Z is not None:
        raise NotImplementedError("factor_condition() on an input is not implemented by the MI355X backend")
    args = _nmf_args(layer, net.config)
    if src.type == "shared":
        if not all(x.type == "input" for x in src.inputs):
            raise NotImplementedError("factor_shared() over layers is not implemented by the MI355X backend (inputs only)")
        data, rows = stack_shared(src.inputs)
        model = _nmf.nmf(data, **args)
        names = [nm if nm else "input%d" % (i + 1) for i, nm in enumerate(src.input_names)]
        Wd, r0 = {}, 0
        for nm, r in zip(names, rows):
            Wd[nm] = model.w[r0:r0 + r]
            r0 += r
        lr = LayerResult(Wd, model.d, model.h, model.misc["iter"], model.misc["loss"], model.misc.get("converged"))
        return FactorNetResult({name: lr}, net.config, True, names, lr.iterations, lr.loss, lr.converged, misc=model.misc)
    if src.type != "input":
        raise ValueError("effective_input: cannot resolve input for first layer")
    model = _nmf.nmf(src.data, **args)
    lr = LayerResult(model.w, model.d, model.h, model.misc["iter"], model.misc["loss"], model.misc.get("converged"))
    return FactorNetResult({name: lr}, net.config, False, None, lr.iterations, lr.loss, lr.converged, misc=model.misc)


def fit(net):
    """R/factor_methods.R:45-72 fit.factor_net."""
    if not isinstance(net, FactorNet):
        raise ValueError("fit() needs a factor_net from factor_net()")
    if net.n_layers == 0:
        raise ValueError("factor_net has no layers to fit")                                              # :49-50
    _refuse_layer_options(net)
    if net.n_layers == 1:
        return _fit_single(net)
    cfg = net.config
    if cfg.resource not in ("auto", "gpu"):
        raise ValueError("rcppml_amd has no CPU path; resource must be 'auto' or 'gpu'")
    desc = deep_descriptor(net)
    extra = dict(cfg.dots)
    r = _abi._check(_abi.factor_net_fit(
        desc["csc"], desc["dense"], desc["m"], desc["n"], desc["rank"], desc["src_kind"], desc["branches"], desc["cond_Z"], desc["L1"],
        desc["L2"], desc["upper_bound"], desc["nonneg"], max_iter=cfg.maxit, tol=cfg.tol, seed=0 if cfg.seed is None else int(cfg.seed),
        solver_mode=solver_mode(cfg), norm_type=_NORMS.index(cfg.norm), cd_maxit=int(extra.get("cd_maxit", 100)),
        cd_tol=float(extra.get("cd_tol", 1e-8))), "factor graph fit")
    layers = {}
    for name, (Wm, dv, Hm) in zip(net.layer_names, r["layers"]):
        # every layer reports the loop's iterations, loss and flag (fit.hpp:362-372)
        layers[name] = LayerResult(Wm, dv, Hm, r["iter"], r["loss"], r["converged"])
    return FactorNetResult(layers, cfg, False, None, r["iter"], r["loss"], r["converged"], layer_losses=r["layer_loss"],
                           misc=dict(counts=r["counts"]))


def predict(result, newdata):
    """R/factor_methods.R:742-777 predict.factor_net_result, single-layer only: project new samples (features x samples) onto the
    trained W through the existing predict(); returns H_new (k x n_new).

    Multi-layer results raise: the reference's chain (:763-776) hands t(H_new) -- n_new x k -- to the next layer's model, which was
    fitted on n_train rows, so it only runs when n_new happens to equal n_train; it is not copied.  Multi-modal results raise as in
    the reference (:752-755)."""
    if not isinstance(result, FactorNetResult):
        raise ValueError("predict() needs a factor_net_result from fit()")
    if result.n_layers != 1:
        raise NotImplementedError("predict() for multi-layer results is not implemented by the MI355X backend")
    lr = next(iter(result.layers.values()))
    if isinstance(lr.W, dict):
        raise ValueError("predict() for multi-modal results requires matching modality structure; concatenate new data in the same order as "
                         "training inputs")
    misc = {key: result.misc[key] for key in ("L1", "L2") if key in result.misc}
    return _nmf.predict(_nmf.NMFModel(lr.W, lr.d, lr.H, misc), newdata)
