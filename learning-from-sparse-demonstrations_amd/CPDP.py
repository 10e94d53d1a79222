"""Host-side mirror of the reference's ``CPDP`` module (CPDP/CPDP.py).

Same classes, method names and argument meaning as the reference —
``COCSys`` (CPDP.py:9-390) and ``COCSys_TimeVarying`` (CPDP.py:394-786) —
with the numerics executed by the model's HIP library on the GPU:

=====================  =====================================================
reference               here
=====================  =====================================================
setDyn/setPathCost/...  keep sympy expressions (symbolic.SX instead of casadi.SX)
diffPMP/raccatiODE/     derivative code is *generated and compiled*
auxSysODE               (codegen.py) instead of building CasADi Functions
cocSolver               lfsd_coc_solve  (IPOPT -> batched DDP, same NLP)
auxSysSolver            lfsd_aux_solve  (solve_ivp BDF/RK45 -> split-step RK4
                        + Richardson on the same ODEs and interpolants)
=====================  =====================================================

Beyond the reference's one-trajectory calls there are ``*Batch`` methods that
keep everything in HBM for thousands of trajectories, and ``SparseDemoLearner``
that runs the outer learning iteration (loss, gradient, parameter update) of
the examples / lib/QuadAlgorithm.py on the device.
"""
import numpy as np
import sympy as sp
import scipy.interpolate as ip
import torch

from . import symbolic, codegen, runtime
from .runtime import LfsdError, ModelLibrary


class COCSys:
    time_varying = False
    # tests / tuning tools: force one mapping of the OC solve for every instance ("lockstep" | "wide"), whatever the
    # instance or the batch size would pick (the C ABI takes the choice as an argument; nothing reads the environment)
    mapping_override = None

    def __init__(self, project_name="myOc"):
        self.sys_name = project_name
        self.time = sp.Symbol('time', real=True)
        self.device = torch.device("cuda", 0) if torch.cuda.is_available() else None
        self.dtype = torch.float32
        self._lib = None
        self._lib_override = None
        self.aux_substeps = 0           # minimum split units per grid interval; 0 = library default (1 with aux_rtol > 0)
        self.aux_rtol = 1e-3            # error-controlled sub-stepping of the auxiliary sweeps at the reference's own
                                        # solve_ivp tolerance (CPDP.py:335, 368: scipy's default rtol); 0: fixed aux_substeps
        self.max_iter = 300              # (IPOPT's default is 3000; an iteration here is one DDP sweep)
        self.tol = None
        self.exact_after = 16            # iteration from which the exact stage Hessian is forced
        self.aux_dtype = None            # None: same as dtype; torch.float64: fp64 auxiliary (Riccati/sensitivity) pass
        self.mapping = "auto"            # "auto" | "lockstep" | "wide": mapping of the OC solve onto the machine
        self.aux_interpolation = "linear"    # "linear": auxSysSolver takes linear interpolants only; "as_given": also the cubic one
        # state bounds (augmented Lagrangian): first penalty, its growth, feasibility tolerance (None: 1e-7 fp64 / 1e-4 fp32,
        # relative to 1 + the largest finite bound), limit of outer iterations
        self.state_rho0, self.state_rho_growth, self.state_tol, self.state_max_outer = 10.0, 10.0, None, 40

    # ---- model definition (CPDP.py:15-87) ------------------------------------------------------
    def setAuxvarVariable(self, auxvar=None):
        if auxvar is None:
            auxvar = symbolic.SX.sym('auxvar')
        self.auxvar = symbolic._flat([auxvar])
        self.n_auxvar = len(self.auxvar)
        self._lib = None

    def setStateVariable(self, state, state_lb=[], state_ub=[]):
        """CPDP.py:20-31: bounds are used only when their length equals n_state (otherwise +-1e20, as the reference).
        Finite state bounds are the variable bounds lbw / ubw of the shooting nodes X_1..X_N in the reference's NLP
        (CPDP.py:140-147; X_0 is pinned to ini_state, :131-134), which IPOPT's interior point handles; here they are
        enforced by an augmented-Lagrangian outer loop around the batched solve (cocSolverBatch): every node gets a
        multiplier pair and a quadratic penalty, the kernels solve the subproblem, the host updates multipliers and penalty
        until the nodes are feasible to `state_tol`."""
        self.state = symbolic._flat([state])
        self.n_state = len(self.state)
        self.state_lb = [float(v) for v in state_lb] if len(state_lb) == self.n_state else self.n_state * [-1e20]
        self.state_ub = [float(v) for v in state_ub] if len(state_ub) == self.n_state else self.n_state * [1e20]
        if any(l > u for l, u in zip(self.state_lb, self.state_ub)):
            raise ValueError("state_lb > state_ub")
        self._lib = None

    def _state_bounds(self):
        """(lb, ub) device tensors, or (None, None) when no bound is finite."""
        lb, ub = getattr(self, "state_lb", None), getattr(self, "state_ub", None)
        if lb is None or not any(abs(v) < 1e19 for v in lb + ub):
            return None, None
        return self._t(lb), self._t(ub)

    def setControlVariable(self, control, control_lb=[], control_ub=[]):
        """CPDP.py:33-46: bounds are used only when their length equals n_control (otherwise +-1e20, as the reference).
        Finite control bounds are honoured by the control-limited backward sweep of the HIP solver."""
        self.control = symbolic._flat([control])
        self.n_control = len(self.control)
        self.control_lb = [float(v) for v in control_lb] if len(control_lb) == self.n_control else self.n_control * [-1e20]
        self.control_ub = [float(v) for v in control_ub] if len(control_ub) == self.n_control else self.n_control * [1e20]
        if any(l > u for l, u in zip(self.control_lb, self.control_ub)):
            raise ValueError("control_lb > control_ub")
        self._lib = None

    def _control_bounds(self):
        """(lb, ub) device tensors, or (None, None) when no bound is finite."""
        lb, ub = getattr(self, "control_lb", None), getattr(self, "control_ub", None)
        if lb is None or not any(abs(v) < 1e19 for v in lb + ub):
            return None, None
        return self._t(lb), self._t(ub)

    def setTimeVariable(self, t=None):
        self.time = t if t is not None else sp.Symbol('time', real=True)

    def setDyn(self, ode):
        if not hasattr(self, 'auxvar'):
            self.setAuxvarVariable()
        self.dyn = sp.Matrix(symbolic._flat([ode]))
        self._lib = None

    def setPathCost(self, path_cost):
        if not hasattr(self, 'auxvar'):
            self.setAuxvarVariable()
        self.path_cost = sp.sympify(path_cost)
        self._lib = None

    def setFinalCost(self, final_cost):
        if not hasattr(self, 'auxvar'):
            self.setAuxvarVariable()
        self.final_cost = sp.sympify(final_cost)
        self._lib = None

    def setInterface(self, interface=None):
        """The interface function y = g(x) of the sparse-demonstration loss as a symbolic expression of the state -- what the
        reference's examples build as ``Function('interface', [oc.state], [expr])`` together with its ``jacobian``
        (lib/QuadAlgorithm.py:616-639, Examples/robotarm_random.py:35-36).  It is compiled into the model library (g and
        (dg/dx)^T r as generated code); ``auxSysSolverBatch`` / ``SparseDemoLearner`` called with ``interface_idx=None`` use
        it.  Interfaces that merely select state components need none of this: pass ``interface_idx``."""
        self.interface = None if interface is None else symbolic._flat([interface])
        self._lib = None

    def setIntegrator(self, n_grid=10, steps_per_grid=4):
        self.n_grid = n_grid
        self.steps_per_grid = steps_per_grid

    # ---- extensions ---------------------------------------------------------------------------
    def setDevice(self, device=None, dtype=None, aux_dtype=None):
        """dtype: arithmetic of the OC solve; aux_dtype (optional): arithmetic of the differentiated-PMP pass, e.g.
        fp32 solve + fp64 Riccati/sensitivity sweeps (BASELINE configs[4])."""
        if device is not None:
            self.device = torch.device(device)
        if dtype is not None:
            self.dtype = dtype
        if aux_dtype is not None:
            self.aux_dtype = aux_dtype

    def setSolverOptions(self, max_iter=None, tol=None, aux_substeps=None, exact_after=None, aux_rtol=None, mapping=None,
                         aux_interpolation=None):
        """aux_interpolation: what ``auxSysSolver(time_grid, opt_sol, theta)`` accepts as ``opt_sol``.  "linear" (default): the linear
        interpolant of its grid values only, anything else is refused.  "as_given": the reference's behaviour (CPDP.py:320-323, 347:
        it integrates along whatever it is handed) for the two interpolants ``cocSolver`` can return -- also the cubic one of
        ``interplation_level=2`` (scipy's not-a-knot spline, from ``interpolation(x, y, 2)`` or a user's own ``CubicSpline``)."""
        if max_iter is not None:
            self.max_iter = int(max_iter)
        if tol is not None:
            self.tol = float(tol)
        if aux_substeps is not None:
            self.aux_substeps = int(aux_substeps)
        if exact_after is not None:
            self.exact_after = int(exact_after)
        if aux_rtol is not None:
            self.aux_rtol = float(aux_rtol)
        if mapping is not None:
            if mapping not in runtime.MAPPINGS:
                raise LfsdError("mapping must be one of %s" % sorted(runtime.MAPPINGS))
            self.mapping = mapping
        if aux_interpolation is not None:
            if aux_interpolation not in ("linear", "as_given"):
                raise LfsdError("aux_interpolation must be 'linear' or 'as_given'")
            self.aux_interpolation = aux_interpolation

    def use_library(self, path_or_lib):
        """Bind an already built model library (tests use this to inject the SIMT-emulator build)."""
        self._lib_override = path_or_lib if isinstance(path_or_lib, ModelLibrary) else ModelLibrary(path_or_lib)
        self._lib = None

    # ---- model -> HIP library -------------------------------------------------------------------
    def model_spec(self, name=None):
        for attr in ('state', 'control', 'dyn', 'path_cost', 'final_cost'):
            assert hasattr(self, attr), {"state": "Define the state variable first!",
                                         "control": "Define the control variable first!",
                                         "dyn": "Define the system dynamics first!",
                                         "path_cost": "Define the running cost/reward function first!",
                                         "final_cost": "Define the final cost/reward function first!"}[attr]
        known = set(self.state) | set(self.control) | set(self.auxvar) | {self.time}
        iface = getattr(self, "interface", None)
        ifree = set().union(*[sp.sympify(g).free_symbols for g in iface]) if iface else set()
        free = (self.dyn.free_symbols | self.path_cost.free_symbols | self.final_cost.free_symbols | ifree) - known
        bad = [s for s in free if not symbolic.is_const(s)]
        if bad:
            raise LfsdError("free symbols that are neither state, control, auxvar nor const(): %s" % bad)
        consts = sorted(free, key=lambda s: int(str(s).rsplit('__k', 1)[1]))
        tv = self.time_varying and (self.time in (self.dyn.free_symbols | self.path_cost.free_symbols |
                                                  self.final_cost.free_symbols))
        return codegen.ModelSpec(self.state, self.control, self.auxvar, consts, self.time, self.dyn, self.path_cost,
                                 self.final_cost, time_varying=tv,
                                 const_defaults=[symbolic.const_default(s) for s in consts],
                                 name=name or self.sys_name, interface=iface)

    def compile(self, force=False, verbose=False):
        if self._lib is not None and not force:
            return self._lib
        spec = self.model_spec()
        if self._lib_override is not None:
            lib = self._lib_override
            if lib.hash != spec.hash():
                raise LfsdError("bound library was built for a different model (%s vs %s)" % (lib.hash, spec.hash()))
        else:
            lib = ModelLibrary(runtime.build_library(spec, force=force, verbose=verbose))
        self._spec = spec
        self._lib = lib
        self.const_values = list(spec.const_defaults)     # this instance's values; the library only fixes the structure
        return lib

    # the reference builds CasADi Functions here (CPDP.py:201-298); for us that is the code generator
    def diffPMP(self):
        self.compile()

    def raccatiODE(self):
        self.compile()

    def auxSysODE(self):
        self.compile()

    # ---- batched device API ------------------------------------------------------------------------
    def _dev(self):
        lib = self.compile()
        if lib.is_emulator:
            return torch.device("cpu")
        if self.device is None or self.device.type != "cuda":
            raise LfsdError("no GPU: the HIP solver has no CPU fallback")
        return self.device

    def _t(self, a, shape=None):
        t = torch.as_tensor(np.asarray(a, dtype=np.float64) if not isinstance(a, torch.Tensor) else a)
        t = t.to(device=self._dev(), dtype=self.dtype)
        if shape is not None:
            t = t.expand(shape) if t.dim() == len(shape) else t.reshape(shape)
        return t.contiguous()

    def consts_tensor(self, batch=None, overrides=None):
        """Runtime constants: shared [n_const] (batch=None) or per-trajectory [B][n_const]."""
        lib = self.compile()
        base = torch.tensor(self.const_values, dtype=torch.float64)
        if overrides:
            names = [str(s).rsplit('__k', 1)[0] for s in self._spec.consts]
            for k, v in overrides.items():
                idx = [i for i, nm in enumerate(names) if nm == k]
                if not idx:
                    raise LfsdError("unknown constant %r (have %s)" % (k, names))
                v = torch.as_tensor(v, dtype=torch.float64)
                if v.dim() == 0:
                    base[idx[0]] = v
                else:
                    if batch is None:
                        batch = v.shape[0]
                    if base.dim() == 1:
                        base = base.repeat(batch, 1)
                    base[:, idx[0]] = v
        if batch is not None and base.dim() == 1:
            base = base.repeat(batch, 1)
        if lib.n_const == 0:
            return None
        return base.to(device=self._dev(), dtype=self.dtype).contiguous()

    def cocSolverBatch(self, ini_state, horizon, auxvar, consts=None, u_init=None, workspace=None, out=None):
        """Solve B problems. ini_state [B,n], horizon scalar or [B], auxvar [B,p] (or [p]) -> dict of device tensors."""
        lib = self.compile()
        if not hasattr(self, 'n_grid'):
            self.setIntegrator()
        x0 = self._t(ini_state)
        if x0.dim() == 1:
            x0 = x0.unsqueeze(0)
        B = x0.shape[0]
        th = self._t(auxvar)
        if th.dim() == 1:
            th = th.unsqueeze(0).expand(B, -1).contiguous()
        hz = self._t(horizon)
        if hz.dim() == 0:
            hz = hz.expand(B).contiguous()
        if consts is None:
            consts = self.consts_tensor()
        clb, cub = self._control_bounds()
        slb, sub = self._state_bounds()
        kw = dict(max_iter=self.max_iter, tol=self.tol, exact_after=self.exact_after,
                  mapping=COCSys.mapping_override or self.mapping)
        if slb is None:
            sol = lib.coc_solve(x0, hz, th, consts, self.n_grid, self.steps_per_grid, u_init=u_init, workspace=workspace,
                                out=out, control_lb=clb, control_ub=cub, **kw)
        else:
            sol = self._solve_state_bounded(lib, x0, hz, th, consts, u_init, workspace, out, clb, cub, slb, sub, kw)
        sol.update(horizon=hz, auxvar=th, consts=consts, ini_state=x0, n_grid=self.n_grid)
        return sol

    def _solve_state_bounded(self, lib, x0, hz, th, consts, u_init, workspace, out, clb, cub, slb, sub, kw):
        """Augmented-Lagrangian outer loop for finite state bounds on the shooting nodes X_1..X_N (CPDP.py:140-147).
        Subproblem k (one lfsd_coc_solve, warm-started from the controls of subproblem k-1): the NLP plus, per node and state
        component, [max(0, lu + rho (x - ub))^2 - lu^2 + max(0, ll + rho (lb - x))^2 - ll^2] / (2 rho).  Then
        lu <- max(0, lu + rho (x - ub)), ll <- max(0, ll + rho (lb - x)); rho grows when the worst violation of the batch
        shrinks by less than 4x.  Done when every node of every trajectory is feasible to `state_tol` and the multipliers
        have stopped moving: the last subproblem's stationarity is then the KKT condition of the bounded NLP, with
        lu - ll the bound multipliers (IPOPT's lam_x) and the returned costates the dynamics multipliers (lam_g).

        Failure is reported per trajectory, as IPOPT would (infeasible problem / iteration limit): when the loop ends
        without meeting that test, every row that is still infeasible beyond `state_tol`, or whose last subproblem did not
        end CONVERGED / STALLED, gets status 3 (MAXITER) -- `mask_unconverged`, `cocSolver` and the tests decide on
        `status` alone.  The reference puts the bounds on X_0 as well (CPDP.py:126-134), so an `ini_state` outside a
        finite box makes its NLP infeasible: that raises here.  The returned `cost` is the AUGMENTED value of the last
        subproblem -- objective + multiplier terms, which at a node that violates its bound by g estimates the optimal value
        to O(g^2) where the plain objective of the (slightly infeasible) iterate is off by lambda g (measured against the
        independent SLSQP solve: 6e-12 against 1.5e-8); `cost_objective` is the plain objective of the returned grids."""
        B, n, N = x0.shape[0], lib.n_state, self.n_grid
        if bool(((x0 < slb) | (x0 > sub)).any()):
            raise LfsdError("ini_state violates the state bounds: the reference's NLP bounds X_0 too (CPDP.py:126-134) "
                            "and is infeasible")
        if clb is None:                     # the bounded kernel reads both boxes
            clb, cub = self._t(lib.n_control * [-1e20]), self._t(lib.n_control * [1e20])
        mult = torch.zeros((B, N, 2, n), dtype=x0.dtype, device=x0.device)
        rho = float(self.state_rho0)
        finite = torch.cat([slb[slb.abs() < 1e19], sub[sub.abs() < 1e19]])
        scale = 1.0 + float(finite.abs().max())
        tol = self.state_tol if self.state_tol is not None else (1e-7 if x0.dtype == torch.float64 else 1e-4)
        viol_prev, iters_total, sol = None, None, None
        met, viol_b = False, None
        for outer in range(int(self.state_max_outer)):
            sol = lib.coc_solve(x0, hz, th, consts, self.n_grid, self.steps_per_grid, u_init=u_init, workspace=workspace,
                                out=out, control_lb=clb, control_ub=cub, state_lb=slb, state_ub=sub, state_mult=mult,
                                state_rho=rho, **kw)
            workspace, out = sol["workspace"], {k: sol[k] for k in ("state_grid", "control_grid", "costate_grid", "cost",
                                                                   "iters", "status")}
            iters_total = sol["iters"].clone() if iters_total is None else iters_total + sol["iters"]
            X = sol["state_grid"][:, 1:, :]
            gu, gl = X - sub, slb - X                                        # <= 0 when feasible
            new_u = torch.clamp(mult[:, :, 0] + rho * gu, min=0.0)
            new_l = torch.clamp(mult[:, :, 1] + rho * gl, min=0.0)
            moved_b = torch.maximum((new_u - mult[:, :, 0]).abs().amax(dim=(1, 2)), (new_l - mult[:, :, 1]).abs().amax(dim=(1, 2)))      # per trajectory
            moved = float(moved_b.max())
            # the plain objective: the node terms the kernel added, at the multipliers and penalty it was called with
            pen = ((torch.clamp(mult[:, :, 0] + rho * gu, min=0.0) ** 2 - mult[:, :, 0] ** 2
                    + torch.clamp(mult[:, :, 1] + rho * gl, min=0.0) ** 2 - mult[:, :, 1] ** 2) / (2.0 * rho)).sum(dim=(1, 2))
            mult = torch.stack((new_u, new_l), dim=2).contiguous()
            viol_b = torch.clamp(torch.maximum(gu, gl), min=0.0).amax(dim=(1, 2))       # per trajectory
            viol = float(viol_b.max())
            solved = bool(((sol["status"] == 1) | (sol["status"] == 2)).all())
            rho_last = rho
            if solved and viol <= tol * scale and moved <= tol * scale * rho:
                met = True
                break
            if viol_prev is not None and viol > 0.25 * viol_prev and rho < 1e8:
                rho *= float(self.state_rho_growth)
            viol_prev = viol
            u_init = sol["control_grid"][:, :-1].contiguous()
        sol["iters"] = iters_total
        sol["cost_objective"] = sol["cost"] - pen.to(sol["cost"].dtype)
        if not met:         # outer-iteration limit or penalty cap: infeasible / non-KKT rows must not pass for solved
            # (a row whose own multipliers were still moving in the last update is not a KKT point of the bounded NLP either,
            #  however feasible and converged its last subproblem was)
            bad = (viol_b > tol * scale) | (moved_b > tol * scale * rho_last) | ~((sol["status"] == 1) | (sol["status"] == 2))
            sol["status"] = torch.where(bad & (sol["status"] != 4), torch.full_like(sol["status"], 3), sol["status"])
        sol["state_mult"], sol["state_rho"], sol["al_outer"], sol["state_violation"] = mult, rho, outer + 1, viol
        sol["state_violation_rows"] = viol_b
        return sol

    def check_waypoints(self, taus, horizon, interface_idx, weights=None):
        """``weights``: waypoint weights in the shape of ``taus``; entries of weight zero do not exist and are exempt (their tau may
        be NaN or outside the horizon).
        Host-side validation the kernels do not repeat.  The reference's opt_sol(t) is scipy's interp1d (CPDP.py:386),
        which raises ValueError for t outside [0, horizon]; its interface functions are arbitrary CasADi expressions,
        ours select state components only."""
        lib = self.compile()
        if interface_idx is None:
            if lib.n_interface == 0:
                raise LfsdError("no interface_idx given and no interface function set (COCSys.setInterface)")
        else:
            idx = [int(i) for i in interface_idx]
            if any(i < 0 or i >= lib.n_state for i in idx):
                raise LfsdError("interface_idx %s outside [0, n_state=%d)" % (idx, lib.n_state))
        self.check_time_range(taus, horizon, weights)

    @staticmethod
    def check_time_range(taus, horizon, weights=None):
        """scipy's interp1d raises ValueError for t outside [0, horizon] (CPDP.py:386); the kernels extrapolate: the check is here.
        ``weights`` (shape of ``taus``, or None): a waypoint of weight zero is never read by the kernels and is not checked."""
        tt = torch.as_tensor(taus, dtype=torch.float64).cpu() if not isinstance(taus, torch.Tensor) else taus.double().cpu()
        hz = torch.as_tensor(horizon, dtype=torch.float64).cpu() if not isinstance(horizon, torch.Tensor) else horizon.double().cpu()
        hz = hz.reshape(-1, 1) if (hz.dim() >= 1 and tt.dim() == 2 and hz.numel() == tt.shape[0]) else hz.min()
        bad = ~((tt >= 0) & (tt <= hz * (1 + 1e-12))) if weights is not None else ((tt < 0) | (tt > hz * (1 + 1e-12)))
        if weights is not None:      # (a NaN tau is outside the range too, unless its weight is zero)
            ww = torch.as_tensor(weights, dtype=torch.float64).cpu() if not isinstance(weights, torch.Tensor) else weights.double().cpu()
            bad = bad & (ww.expand_as(tt) != 0)
        if tt.numel() and bool(bad.any()):
            raise ValueError("A value in taus is outside the interpolation range [0, horizon].")

    @staticmethod
    def check_weights(weights):
        """Waypoint weights must be finite and non-negative (the kernels do not check: include/lfsd_cpdp.h, ABI 16).  One host read."""
        ww = torch.as_tensor(weights, dtype=torch.float64).cpu() if not isinstance(weights, torch.Tensor) else weights.double().cpu()
        if ww.numel() and not bool((torch.isfinite(ww) & (ww >= 0)).all()):
            raise LfsdError("waypoint weights must be finite and non-negative")

    def auxSysSolverBatch(self, sol, taus=None, waypoints=None, interface_idx=None, auxvar=None, want_grids=False,
                          Z_grid=None, out=None, phase_hook=None, validate=True, skip_status=None, interplation_level=1,
                          waypoint_weights=None, auxX_grid=None, auxU_grid=None):
        """Differentiate the PMP along ``sol`` and (optionally) evaluate the sparse-waypoint loss + gradient.
        ``Z_grid``, ``auxX_grid``, ``auxU_grid``: the caller's buffers for [P W] and (with ``want_grids``) the sensitivity grids.
        ``waypoint_weights`` ([K] or [B, K], default None = every waypoint counts once, the launches as ever): loss =
        sum_k w_k |y(tau_k) - wp_k|^2 and its gradient from the weighted forward sweep (``lfsd_aux_forward[_cubic]_weighted``).  A
        weight of zero removes the waypoint: its tau and target are never read and may be NaN padding (``pad_demonstrations``).
        Weights are checked (finite, non-negative) with ``validate``.
        ``interplation_level`` (the reference's spelling, CPDP.py:92): 1 -- along the linear interpolant of the solved grids, what
        ``cocSolver`` returns by default; 2 -- along their cubic interpolant (``cocSolver(..., interplation_level=2)``, CPDP.py:388-390):
        the curvature grids are fitted on the device (``lfsd_grid_curvature``) and the sweeps run the ``*_cubic`` entry points.
        ``skip_status``: OC-solve statuses whose rows are NOT differentiated (NaN loss / gradient, no sweep).  Default:
        FAILED (4) only -- a solve that ended with non-finite grids has nothing to differentiate and would otherwise hold
        the launch at the refinement cap; a solve at the iteration limit (3) is differentiated as the reference does,
        unless the caller (SparseDemoLearner with skip_unconverged) says otherwise."""
        lib = self.compile()
        B = sol["state_grid"].shape[0]
        th = sol["auxvar"] if auxvar is None else self._t(auxvar, (B, lib.n_auxvar))
        tt = wp = ii = ww = None
        if taus is None and waypoint_weights is not None:
            raise LfsdError("waypoint_weights without waypoints")
        if taus is not None:
            tt = self._t(taus)
            if tt.dim() == 1:
                tt = tt.unsqueeze(0).expand(B, -1).contiguous()
            if waypoint_weights is not None:
                ww = self._t(waypoint_weights)
                if ww.dim() == 1:
                    ww = ww.unsqueeze(0).expand(B, -1)
                if tuple(ww.shape) != tuple(tt.shape):
                    raise LfsdError("waypoint_weights has shape %s: [K] or [B, K] = %s as taus" % (tuple(ww.shape), tuple(tt.shape)))
                ww = ww.contiguous()
                if validate:
                    self.check_weights(ww)
            wp = self._t(waypoints)
            if wp.dim() == 2:
                wp = wp.unsqueeze(0).expand(B, -1, -1).contiguous()
            ii = None if interface_idx is None else torch.as_tensor(list(interface_idx), dtype=torch.int32, device=self._dev())
            if validate:          # (a device->host read: callers that validated at setup switch it off)
                self.check_waypoints(tt, sol["horizon"], interface_idx, ww)
        hz, cs, X, U, Lm = sol["horizon"], sol["consts"], sol["state_grid"], sol["control_grid"], sol["costate_grid"]
        ad = self.aux_dtype
        if ad is not None and ad != X.dtype:          # mixed precision: promote the solved grids for the aux pass
            cv = lambda t: None if t is None else t.to(ad).contiguous()
            hz, th, cs, X, U, Lm, tt, wp, ww = (cv(t) for t in (hz, th, cs, X, U, Lm, tt, wp, ww))
        status = sol.get("status")
        if skip_status is None:
            skip_status = (4,)
        if status is None:
            skip_status = ()
        return lib.aux_solve(hz, th, cs, X, U, Lm, tt, wp, ii, substeps=self.aux_substeps, want_grids=want_grids,
                             Z_grid=Z_grid, out=out, phase_hook=phase_hook, rtol=self.aux_rtol, oc_status=status,
                             skip_status=skip_status, interp_level=interplation_level, auxX_grid=auxX_grid, auxU_grid=auxU_grid,
                             **({} if ww is None else dict(wp_weight=ww)))

    def _times(self, times, dtype, batch):
        tt = times if isinstance(times, torch.Tensor) else torch.as_tensor(np.asarray(times, dtype=np.float64))
        tt = tt.to(device=self._dev(), dtype=dtype)
        if tt.dim() == 0:
            tt = tt.reshape(1)
        if tt.dim() not in (1, 2) or (tt.dim() == 2 and tt.shape[0] != batch):
            raise LfsdError("times must be [K] (shared by the batch) or [B, K], got %s" % (tuple(tt.shape),))
        return tt.contiguous()

    def sampleBatch(self, sol, times, interplation_level=1, validate=True):
        """``opt_sol(times)`` of every trajectory of ``sol`` (cocSolverBatch), on the device: what the reference's examples call to make
        demonstrations and final trajectories (Examples/rocket_groundtruth.py:75-84, lib/QuadAlgorithm.py:306-317) and inside their
        loss functions.  times [K] (shared) or [B, K] -> dict(state [B,K,n], control [B,K,m], costate [B,K,n]).
        ``interplation_level`` 1: the linear interpolant of the grids (CPDP.py:386); 2: their cubic one (CPDP.py:388-390) -- the
        curvature grids are taken from ``sol["curvature"]`` (state, control, costate) if present, else fitted (``lfsd_grid_curvature``).
        ``validate``: times outside [0, horizon] raise ValueError as scipy's interp1d does (a device->host read); without it
        they extrapolate the end interval."""
        lib = self.compile()
        if interplation_level not in (1, 2):
            raise LfsdError("interplation_level must be 1 (linear) or 2 (cubic), got %r" % (interplation_level,))
        grids = (sol["state_grid"], sol["control_grid"], sol["costate_grid"])
        dt, B = grids[0].dtype, grids[0].shape[0]
        hz = sol["horizon"].to(dt)
        tt = self._times(times, dt, B)
        if validate:
            self.check_time_range(tt, hz)
        curv = (None, None, None)
        if interplation_level == 2:
            curv = sol.get("curvature")
            if curv is None or any(c.dtype != dt for c in curv):
                curv = tuple(lib.grid_curvature(g) for g in grids)
        return {k: lib.sample_grid(g, hz, tt, curv=c) for k, g, c in zip(("state", "control", "costate"), grids, curv)}

    def sampleAuxBatch(self, aux, horizon, times, validate=True):
        """``auxsys_sol(times)`` of every trajectory of ``aux`` (auxSysSolverBatch(..., want_grids=True)), on the device:
        dict(dx [B,K,p,n] = dx/dtheta, du [B,K,p,m] = du/dtheta), parameter-major as the grids are (the reference's vector is the
        [n][p] row-major transpose, CPDP.py:352-381).  Linear at either interpolation level, as the reference's (CPDP.py:381)."""
        lib = self.compile()
        aX, aU = aux.get("auxX_grid"), aux.get("auxU_grid")
        if aX is None or aU is None:
            raise LfsdError("sampleAuxBatch needs the sensitivity grids: auxSysSolverBatch(..., want_grids=True)")
        B, N1, p, n = aX.shape
        m = aU.shape[3]
        dt = aX.dtype
        hz = self._t(horizon).to(dt)
        hz = hz.expand(B).contiguous() if hz.dim() == 0 else hz
        tt = self._times(times, dt, B)
        if validate:
            self.check_time_range(tt, hz)
        K = tt.shape[-1]
        return dict(dx=lib.sample_grid(aX.reshape(B, N1, p * n), hz, tt).reshape(B, K, p, n),
                    du=lib.sample_grid(aU.reshape(B, N1, p * m), hz, tt).reshape(B, K, p, m))

    # ---- the reference's one-trajectory calls --------------------------------------------------------
    def cocSolver(self, ini_state, horizon, auxvar_value=1, interplation_level=1, print_level=0):
        """CPDP.py:92-198: returns (time_grid, opt_sol) with opt_sol(t) -> [x, u, lambda]."""
        if not hasattr(self, 'n_grid'):
            self.setIntegrator()
        if type(ini_state) is list:
            ini_state = np.array(ini_state).flatten()
        e = np.atleast_1d(np.asarray(auxvar_value, dtype=np.float64)).ravel()
        sol = self.cocSolverBatch(np.asarray(ini_state, dtype=np.float64)[None, :], float(horizon), e[None, :])
        self.last_solution = sol
        st = int(sol["status"][0])
        if print_level:
            print("lfsd coc_solve: status=%s iters=%d cost=%g" % (runtime.STATUS.get(st, st), int(sol["iters"][0]),
                                                                 float(sol["cost"][0])))
        time_grid = np.linspace(0, float(horizon), self.n_grid + 1)
        grids = np.concatenate([sol[k][0].double().cpu().numpy() for k in ("state_grid", "control_grid",
                                                                           "costate_grid")], axis=1)
        return time_grid, self.interpolation(time_grid, grids, interplation_level)

    def auxSysSolver(self, time_grid, opt_sol, auxvar_value=1):
        """CPDP.py:301-381: returns auxsys_sol(t) -> [vec(dx/dtheta) (n*p, row-major), vec(du/dtheta) (m*p)]."""
        lib = self.compile()
        n, m, p = lib.n_state, lib.n_control, lib.n_auxvar
        # The reference integrates the auxiliary ODEs along WHATEVER interpolant it is handed (CPDP.py:320, 347).  The sweeps here
        # know two: the LINEAR interpolant of the grid values (interplation_level 1, what every example uses) and the CUBIC one of
        # cocSolver(..., interplation_level=2) (CPDP.py:388-390: scipy's not-a-knot spline).  By default only the first is taken and a
        # cubic opt_sol is refused -- it must not silently be resampled to the linear one; setSolverOptions(aux_interpolation=
        # "as_given") differentiates along either.  Anything else is refused under both settings.
        # (interpolation() tags what it returns with `lfsd_level`; an interpolant from elsewhere is probed instead: a piecewise-linear
        #  one is reproduced by the linear interpolant of its own grid values at the interval midpoints, the not-a-knot spline by
        #  that spline of its own grid values.  Nothing relies on scipy's private attributes.)
        level = getattr(opt_sol, "lfsd_level", None)
        if level is None:
            tg_ = np.asarray(time_grid, dtype=np.float64)
            mid = 0.5 * (tg_[:-1] + tg_[1:])
            gv = np.asarray(opt_sol(tg_), dtype=np.float64)
            gm = np.asarray(opt_sol(mid), dtype=np.float64)
            lin = 0.5 * (gv[:-1] + gv[1:])
            thr = 1e-9 * max(1.0, np.abs(gv).max())
            level = "unknown"
            if np.abs(gm - lin).max() <= thr:
                level = 1
            elif len(tg_) >= 4 and np.abs(np.diff(tg_) - (tg_[-1] - tg_[0]) / (len(tg_) - 1)).max() <= 1e-9 * abs(tg_[-1] - tg_[0]):
                c = notaknot_curvature(gv)
                if np.abs(gm - (lin - 0.375 * (c[:-1] + c[1:]))).max() <= thr:      # ((1/2)^3 - 1/2 = -3/8 on both curvatures)
                    level = 2
        if level == 2 and self.aux_interpolation != "as_given":
            raise LfsdError("auxSysSolver: opt_sol is the cubic interpolant of its grid (interplation level 2); by default the HIP sweeps "
                            "take the linear interpolant (interplation_level=1, CPDP.py:386) only -- "
                            "setSolverOptions(aux_interpolation='as_given') differentiates along the cubic one")
        if level not in (1, 2):
            raise LfsdError("auxSysSolver: opt_sol is neither the linear interpolant of its grid (interplation level 1, CPDP.py:386) nor "
                            "its not-a-knot cubic spline (level 2, CPDP.py:388-390; needs setSolverOptions(aux_interpolation="
                            "'as_given')): the HIP sweeps integrate along these two only (level %r)" % (level,))
        time_grid = np.asarray(time_grid, dtype=np.float64)
        N = len(time_grid) - 1
        g = np.asarray(opt_sol(time_grid), dtype=np.float64)
        e = np.atleast_1d(np.asarray(auxvar_value, dtype=np.float64)).ravel()
        sol = dict(state_grid=self._t(g[None, :, 0:n]), control_grid=self._t(g[None, :, n:n + m]),
                   costate_grid=self._t(g[None, :, n + m:]), horizon=self._t([time_grid[-1] - time_grid[0]]),
                   auxvar=self._t(e[None, :]), consts=self.consts_tensor())
        aux = self.auxSysSolverBatch(sol, want_grids=True, interplation_level=level)
        self.last_aux = aux
        X = aux["auxX_grid"][0].double().cpu().numpy().transpose(0, 2, 1).reshape(N + 1, n * p)
        U = aux["auxU_grid"][0].double().cpu().numpy().transpose(0, 2, 1).reshape(N + 1, m * p)
        return self.interpolation(time_grid, np.concatenate((X, U), axis=1))

    def interpolation(self, x, y, method=1):
        """CPDP.py:384-390."""
        if method == 1:
            f = ip.interp1d(x, y, axis=0)
        elif method == 2:
            f = ip.interp1d(x, y, axis=0, kind='cubic')
        else:
            return None                     # (the reference falls off the end of its ifs as well)
        f.lfsd_level = method              # read by auxSysSolver (level 2 is differentiated along under aux_interpolation="as_given")
        return f


def notaknot_curvature(y):
    """Curvatures c_k = h^2 y''(t_k) / 6 of scipy's interp1d(kind='cubic') -- the not-a-knot cubic spline -- through the rows of
    y [N+1, ...] on a uniform grid, N >= 3 (host restatement in fp64 of csrc/cpdp_spline.h; used to recognise such an interpolant).
    With d_k = y_k-1 - 2 y_k + y_k+1:  c_1 = d_1 / 6, c_N-1 = d_N-1 / 6, the (1,4,1) system for c_2 .. c_N-2 between them, and
    c_0 = 2 c_1 - c_2, c_N = 2 c_N-1 - c_N-2."""
    y = np.asarray(y, dtype=np.float64)
    N = y.shape[0] - 1
    if N < 3:
        raise LfsdError("the cubic interpolant needs n_grid >= 3 (four nodes)")
    d = y[:-2] - 2.0 * y[1:-1] + y[2:]               # d[k-1] = d_k
    c = np.zeros_like(y)
    c[1], c[N - 1] = d[0] / 6.0, d[N - 2] / 6.0
    if N >= 5:
        A = np.diag(np.full(N - 3, 4.0)) + np.diag(np.ones(N - 4), 1) + np.diag(np.ones(N - 4), -1)
        rhs = d[1:N - 2].copy()
        rhs[0] = rhs[0] - c[1]
        rhs[-1] = rhs[-1] - c[N - 1]
        c[2:N - 1] = np.linalg.solve(A, rhs.reshape(N - 3, -1)).reshape(rhs.shape)
    elif N == 4:
        c[2] = (d[1] - c[1] - c[3]) / 4.0
    c[0] = 2.0 * c[1] - c[2]
    c[N] = 2.0 * c[N - 1] - c[N - 2]
    return c


class COCSys_TimeVarying(COCSys):
    """CPDP.py:394-786 — dynamics / costs may depend on the time symbol given to ``setTimeVariable``."""
    time_varying = True


def pad_demonstrations(taus_list, waypoints_list, weights_list=None):
    """Ragged demonstrations as one batch: ``taus_list[d]`` (K_d times) and ``waypoints_list[d]`` ([K_d, n_iface] targets), optionally
    ``weights_list[d]`` (K_d weights; default 1 each), padded to K = max K_d.  Returns float64 numpy arrays ``(taus [D, K], waypoints
    [D, K, n_iface], weights [D, K])``: the padding has weight 0 and NaN in ``taus`` and ``waypoints``.  The NaN is deliberate -- a
    waypoint of weight zero is never read by the kernels (include/lfsd_cpdp.h, ABI 16), and a kernel that did read one would show.
    Hand the three to ``SparseDemoLearner(..., taus, waypoints, ..., waypoint_weights=weights)`` or ``auxSysSolverBatch``."""
    D = len(taus_list)
    if D == 0 or len(waypoints_list) != D or (weights_list is not None and len(weights_list) != D):
        raise LfsdError("pad_demonstrations takes one entry per demonstration in every list (got %d, %d%s)"
                        % (D, len(waypoints_list), "" if weights_list is None else ", %d" % len(weights_list)))
    tl = [np.asarray(t, dtype=np.float64).reshape(-1) for t in taus_list]
    wl = []
    for d, (w, t) in enumerate(zip(waypoints_list, tl)):
        w = np.asarray(w, dtype=np.float64)
        if len(t) == 0:
            w = np.zeros((0, 0))
        elif w.ndim != 2 or w.shape[0] != len(t) or w.shape[1] == 0:
            raise LfsdError("demonstration %d: %d times and targets of shape %s ([K_d, n_iface])" % (d, len(t), w.shape))
        wl.append(w)
    ni = max(w.shape[1] for w in wl)
    K = max(len(t) for t in tl)
    if K == 0 or ni == 0:
        raise LfsdError("pad_demonstrations: no demonstration has a waypoint")
    taus, wps, wts = np.full((D, K), np.nan), np.full((D, K, ni), np.nan), np.zeros((D, K))
    for d, (t, w) in enumerate(zip(tl, wl)):
        k = len(t)
        if k and w.shape != (k, ni):
            raise LfsdError("demonstration %d: %d times and targets of shape %s (interface of %d outputs)" % (d, k, w.shape, ni))
        wt = np.ones(k) if weights_list is None else np.asarray(weights_list[d], dtype=np.float64).reshape(-1)
        if len(wt) != k:
            raise LfsdError("demonstration %d: %d times and %d weights" % (d, k, len(wt)))
        taus[d, :k], wts[d, :k] = t, wt
        if k:
            wps[d, :k] = w
    COCSys.check_weights(wts)
    return taus, wps, wts


def chord_length_times(points, average_speed):
    """Time stamps for a polyline flown at a constant speed, as the reference's human-input path invents them
    (lib/InputWaypoints.py:212-228, ``generate_time``): ``points`` [P, d] are the start, the waypoints and the goal; every segment
    takes its chord length divided by ``average_speed``, rounded to 0.01, and the stamps are the running sum from 0.  Returns [P]
    float64: ``[0]`` is 0, ``[1:-1]`` are the waypoint times, ``[-1]`` is the horizon.  Such times are guesses: what
    ``SparseDemoLearner(learn_taus=True)`` corrects."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[0] < 2:
        raise LfsdError("points is [P, d] with P >= 2: start, waypoints, goal (got shape %s)" % (pts.shape,))
    speed = float(average_speed)
    if not (np.isfinite(speed) and speed > 0):
        raise LfsdError("average_speed must be positive and finite (got %r)" % (average_speed,))
    out = np.zeros(pts.shape[0], dtype=np.float64)
    for i in range(1, pts.shape[0]):
        out[i] = round(float(np.linalg.norm(pts[i] - pts[i - 1])) / speed, 2) + out[i - 1]
    return out


class SparseDemoLearner:
    """The outer learning iteration of the examples, batched on the device.

    One iteration (Examples/robotarm_random.py:67-73, lib/QuadAlgorithm.py:454-578):
        solve OC at theta -> differentiate PMP -> waypoint loss & gradient -> parameter update -> projection.
    ``mode='independent'``: every trajectory (seed) owns its theta and optimizer state.
    ``mode='shared'``: one theta for all demonstrations; the gradient is summed over the batch and
    all-reduced over ``process_group`` (RCCL) before a single update.

    ``skip_unconverged`` (default: OFF in ``independent`` mode = the reference's behaviour, every gradient is applied
    to its own seed; ON in ``shared`` mode, where ONE non-finite or unconverged demonstration would otherwise be summed,
    all-reduced and applied to the single theta of every rank).  When switched on, a
    trajectory whose optimal-control solve ended at the iteration limit or failed, or whose loss / gradient is not
    finite, is frozen for that step: its row is masked out of the update kernel (parameters AND optimizer state stay
    untouched, for every update rule), in shared mode it is left out of the summed loss / gradient, and the number of
    dropped demonstrations is all-reduced and reported as ``n_unconverged``.  At the next outer iteration such a solve
    is continued from the controls it stopped at; every other trajectory cold-starts as in the reference.

    ``event_hook(name)``, if set, is called right before each device phase of ``step`` ("oc_solve", "aux_riccati",
    "aux_forward", "update") and once after the last one ("end"), so a caller can bracket the kernels with HIP events
    (bench.py) without re-implementing the iteration.

    ``stop_rule`` (``independent`` mode only; default ``None`` = no rule, the iteration above and nothing else):
    ``dict(loss=0.9, grad_norm=0.05)`` gives every seed the reference loop's own stop test (lib/QuadAlgorithm.py:239-257: go on
    while ``loss > 0.9 and norm(diff_loss) > 0.05``; the reference learns its seeds one at a time, Examples/robotarm_random.py:
    60-73).  The test runs on the device after each update (``lfsd_stop_compact``: test + stable compaction of the seeds still
    learning, one launch; the host reads one int, their number).  A seed that fails it has had its last update -- the reference
    updates, then tests at the top of the next iteration -- and is frozen from then on: ``theta`` / ``m`` / ``v`` / ``vhat`` stay
    [B, p] and its row is masked out of ``lfsd_optimizer_step``.  Once seeds have stopped, the solve and both sweeps run on a DENSE
    batch of the others (``lfsd_gather_rows`` in, ``lfsd_scatter_rows`` out; inputs that do not change are gathered again only
    when the set shrank; with ``warm_start`` / ``skip_unconverged`` a seed's previous controls move with it), mapped onto the
    machine as ``lfsd_coc_solve`` maps a batch of that size.  ``active`` [B] bool, ``stop_iter`` [B] (iterations a stopped seed
    took; 0 = still learning) and ``n_active`` report the state; ``step`` returns full-size (loss, grad) in which a stopped seed
    keeps its last values, and launches nothing once ``n_active == 0``.  A loop timed with the rule on pays that one host read per
    step.

    ``interplation_level`` (the reference's spelling; default 1): 2 differentiates every step along the cubic interpolant of the
    solved grids (``cocSolver(..., interplation_level=2)`` handed to ``auxSysSolver``, CPDP.py:388-390) instead of the linear one;
    one more small launch per grid and step (``lfsd_grid_curvature``).  Every other option combines with it.

    ``loss_fn`` (default ``None`` = the fused waypoint loss above, launch for launch): a user-written loss, as every example of the
    reference ends in one (Examples/pendulum_timewarping.py:72-86, rocket_groundtruth.py:45-70, lib/QuadAlgorithm.py:616-673).
    ``loss_fn(x_tau [B,K,n], u_tau [B,K,m]) -> loss [B]`` is any differentiable torch function of the states and controls at the
    learner's ``taus`` (weights, ragged demonstrations as masks, Huber or geodesic distances, control terms; targets are its own
    business: ``waypoints`` and ``interface_idx`` may be ``None``).  Per evaluation: the solve; the two sweeps with the sensitivity
    grids written and no waypoints; ``sampleBatch`` at ``taus`` on the interpolant of ``interplation_level``; ``loss_fn`` under
    autograd, which yields dL/dx(tau_k), dL/du(tau_k); ``lfsd_waypoint_vjp`` contracts them with the linear interpolants of the
    sensitivity grids (``auxsys_sol`` is linear at either level, CPDP.py:381); the gradient is multiplied by ``grad_scale``.
    ``grad_scale=1`` is the true derivative of ``loss_fn``.  The fused loss follows the reference's "no factor 2" convention
    (lib/QuadAlgorithm.py:630-637: loss |r|^2, gradient r . dx/dtheta): it is ``loss_fn = ((x_tau[:, :, idx] - wp) ** 2).sum((1, 2))``
    with ``grad_scale=0.5``.  It combines with both modes, ``warm_start``, ``skip_unconverged`` (a skipped row's grids are NaN, so are
    its loss and gradient, and ``mask_unconverged`` freezes it), ``true_loss_print_flag`` and both interpolation levels.  Together
    with ``stop_rule`` it is refused for now: the dense batch of the seeds still learning would have to hand ``loss_fn`` its row ids.

    Hyper-parameter sweeps in one batch (``independent`` mode).  The reference's comparison scripts run one problem under several
    update rules or learning rates, one ``QuadAlgorithm.run`` each (test/opt_methods_comparison.py, test/*_learning_rate_comparison.py).
    Here ``method`` may be a sequence of B strings, ``learning_rate`` / ``mu`` / ``beta_1`` / ``beta_2`` / ``epsilon`` each a scalar or
    a length-B sequence, array or tensor, and ``true_loss_print_flag`` a bool or B bools (it acts on Nesterov rows only, as ever).
    With every one of them scalar the learner takes the launches it always took.  ANY sequence selects the rows path: the values
    are assembled as ``hyper`` [B, 5] in fp64 and cast once to theta's dtype -- the numbers ``lfsd_optimizer_step`` gets by casting
    its double arguments; the evaluation point comes from ``lfsd_lookahead_rows`` (skipped when no row is Nesterov) and the update is
    ``lfsd_optimizer_step_rows``.  A row walks, bit for bit, the path it walks in a uniform learner with its configuration.  If any
    Nesterov row has the true-loss flag, the (active) batch is evaluated a second time at theta -- the WHOLE batch, a second solve
    and two more sweeps -- and only the flagged rows take their loss and gradient from it; every other row is left as its uniform
    learner, which has no second evaluation, leaves it: the controls and status its next solve starts from (``warm_start`` /
    ``skip_unconverged``) and its entry of the frozen-row mask the stop test reads stay the first evaluation's.  The arrays stay [B], indexed by original
    row, through ``stop_rule``; the rows path also combines with ``loss_fn``, ``interplation_level``, ``warm_start`` and
    ``skip_unconverged``.  A wrong length or ``mode='shared'`` with a per-row argument (there is one theta) raises ``LfsdError``.

    ``trace`` (default ``None``; both modes): ``trace=capacity`` keeps the traces the reference's loop appends to host lists
    (lib/QuadAlgorithm.py:244-252) on the device: ``loss_trace`` and ``grad_norm_trace`` [B, capacity], ``theta_trace``
    [B, capacity+1, p], filled with NaN, ``theta_trace[:, 0]`` = theta_0.  One ``lfsd_trace_append`` per step files what ``step()``
    returns and theta after the projection; nothing is read back.  With a stop rule the launch gets the seeds active as of the
    previous test: a seed is traced in the step in which it stops and never after -- its later entries stay NaN, as the reference's
    trace simply ends there (a row ``skip_unconverged`` froze for one step is traced: it repeats its theta).  A step beyond the
    capacity raises ``LfsdError``.  In ``shared`` mode the traces have the single row.

    ``method="LM"`` (``independent`` mode, the fused loss): a Levenberg-Marquardt outer update where the reference has first-order rules
    only.  The fused loss is a sum of squares and the forward sweep already returns dx/dtheta on the grid, so every evaluation also
    writes the sensitivity grids and one more small launch (``lfsd_normal_matrix``) forms the Gauss-Newton matrix ``H = J^T J`` [B, p, p]
    of the waypoint residuals, in the sweeps' dtype, cast to theta's as the gradient is.  ``lfsd_lm_step`` then, per row and without a
    host read: accepts the evaluated point iff its loss is below the accepted one and loss, gradient and H are finite (the damping
    ``lambda`` is multiplied by ``lm_down`` on acceptance, by ``lm_up`` on rejection, kept inside [``lm_min``, ``lm_max``]), and solves
    ``(H + lambda (diag H + 1e-8 max diag H I)) delta = -grad`` at the accepted point for the next trial point (projected as ever).
    Defaults ``lm_lambda0=1e-2, lm_down=1/3, lm_up=2, lm_min=1e-8, lm_max=1e8``: ordinary Marquardt values, nothing tuned.
    ``theta`` is the ACCEPTED point; ``step()`` evaluates the trial point and returns its (loss, grad) -- the convention of Nesterov's
    look-ahead point; the first finite evaluation (of theta_0) is always accepted.  ``lm_lambda`` [B], ``lm_loss`` [B] (the accepted
    loss, +inf before the first acceptance; it never increases), ``lm_accepted`` [B] bool (the last step) and ``normal_matrix``
    [B, p, p] (H at the accepted point: small eigenvalues are directions of theta the waypoints do not pin down) report the state.
    It combines with ``stop_rule`` (the test reads the returned loss and gradient), ``warm_start``, ``skip_unconverged`` (a frozen row
    keeps its whole LM state and evaluates the same trial point again -- so a row frozen by its sweeps' tolerance flag, not by an
    unfinished solve, stays frozen: DESIGN.md section 14), ``interplation_level=2`` and ``trace`` (``theta_trace`` files
    the accepted theta).  Refused with ``LfsdError``: ``loss_fn`` (a general loss is not a sum of squares), ``mode='shared'``, any
    per-row argument or a ``method`` sequence containing "LM" (the rows path carries the five first-order rules), a model whose
    interface function is compiled in (``interface_idx=None``: J would need the generated dg/dx), and more than 16 parameters.

    ``mode='grouped', demos_per_seed=D``: G seeds (or configurations) that each learn from the same D demonstrations, B = G * D rows,
    row ``g * D + d`` = demonstration d of group g (``n_groups``, ``demos_per_seed``).  ``ini_state`` / ``horizon`` / ``taus`` /
    ``waypoints`` may be given per demonstration (leading dimension D: tiled over the groups), per row (B) or broadcast as ever;
    ``theta0`` is [p], [1, p] or [G, p].  ``theta``, ``m``, ``v``, ``vhat``, the LM state and the traces have G rows.  One step: the
    evaluation point on G rows, ``lfsd_gather_rows`` to [B, p], the solve and both sweeps (and ``lfsd_normal_matrix``) on B rows as
    ``evaluate()`` runs them in the other modes, ``lfsd_group_reduce`` -- per group 0 plus its rows' loss, gradient and H, added in
    ascending order on the device, the same bits in any batch -- and the unchanged update kernel on G rows.  ``step()`` and
    ``evaluate(theta [G, p])`` return the group sums (loss [G], grad [G, p]); ``row_loss`` [B] / ``row_grad`` [B, p] hold the last
    per-demonstration values, ``n_ok`` [G] int32 (a device tensor) the demonstrations that entered each sum.  ``skip_unconverged``
    defaults to ON, as in shared mode (one bad demonstration would poison a sum): the mask of ``mask_unconverged`` is the kernel's
    ``row_ok``, a group with ``n_ok == 0`` is masked out of the update (parameters, optimizer and LM state keep every word), and
    ``n_unconverged`` counts the rows left out (read only with ``count_unconverged``).  Update rules: the five uniform ones, the rows
    path with sequences of length G, and ``method='LM'`` with H_g the sum of the demonstrations' H (``normal_matrix`` [G, p, p]).  It
    combines with ``warm_start`` (controls stay per row), ``interplation_level=2``, ``loss_fn`` (which sees all B rows), ``trace``
    (G rows) and a scalar ``true_loss_print_flag`` (a second evaluation, reduced as the first).  ``event_hook`` gets one more phase,
    "group_reduce".  Refused with ``LfsdError``: ``stop_rule`` (dense-batch bookkeeping per group), a ``process_group`` or an
    initialised ``torch.distributed`` (no all-reduce is issued), a sequence for ``true_loss_print_flag``, a batch that is no whole
    number of groups, ``demos_per_seed`` with another mode, a ``theta0`` or per-group sequence of the wrong length (DESIGN.md
    section 15).

    ``waypoint_weights`` / ``n_waypoints`` (default ``None`` for both = every waypoint counts once, the launches the learner always
    made, through the unweighted entry points): a weight per waypoint in the fused loss, ``loss = sum_k w_k |y(tau_k) - wp_k|^2`` with
    its gradient and, for ``method="LM"``, ``H = sum_k w_k J_k^T J_k`` (``lfsd_aux_forward[_cubic]_weighted``,
    ``lfsd_normal_matrix_weighted``; the same number of launches).  Weights come in the shapes ``taus`` comes in -- [K], [B, K], in
    grouped mode [D, K] tiled over the seeds -- and are checked once, here: finite and non-negative.  A weight of ZERO removes the
    waypoint: its ``tau`` and target are never read (they may be NaN or outside the horizon) and it adds no operation to any sum, so a
    row that keeps k of its K waypoints walks, bit for bit, the path it walks in a learner built with those k alone -- ragged
    demonstrations share one batch (``pad_demonstrations`` pads Python lists with NaN and weight 0).  ``n_waypoints`` (integers: a
    scalar, [B], or [D] in grouped mode) is shorthand for weight 1 below the count and 0 from it on.  All-ones weights give the bits
    of no weights.  It combines with the three modes (in shared mode the all-reduce still carries p + 2 numbers), the five rules, the
    rows path and ``"LM"``, ``interplation_level=2``, ``warm_start``, ``skip_unconverged``, ``trace``, ``true_loss_print_flag`` (the
    second evaluation uses the same weights) and ``stop_rule`` (the weights move to the dense batch with ``taus`` and ``waypoints``).
    Refused with ``LfsdError``: together with ``loss_fn`` (a user loss does its own weighting), both arguments at once, negative or
    non-finite weights, a shape that is none of the above, a count outside [0, K].

    ``learn_taus`` (default ``False`` = the times are data, the launches, buffers and bits the learner always had): the waypoint times
    are learned beside theta.  They are guesses in the reference too -- its human-input path builds them from chord length over an
    average speed (lib/InputWaypoints.py:212-228, ``chord_length_times``) -- and the time-warp parameter can only stretch them all by
    one factor.  Every row owns its times [B, K] in all three modes (in shared and grouped mode each demonstration row keeps its own;
    nothing about them is reduced or all-reduced).  One step: the evaluation at (theta point, tau point) through the unchanged fused
    path; ``lfsd_waypoint_time_grad`` on the solved state grid (at level 2 with its curvature grid) gives
    ``tau_grad[b, k] = w_k r^T dy/dx xdot(tau_k) + tau_prior (tau_k - tau0[b, k])``, no factor 2, as the fused gradient; the theta
    update as ever; ``lfsd_optimizer_step`` on ``taus`` with moments of their own (``m_tau``, ``v_tau``, ``vhat_tau``) under
    ``tau_method`` (default: ``method``, or "Vanilla" when that is a per-row list; momentum and Adam constants are the learner's
    scalars) at ``tau_learning_rate`` (required: times and parameters have different units); ``lfsd_tau_project`` against the times
    the step started from: a time moves by at most ``tau_max_shift`` (in (0, 0.5), default 0.25) of the gap to its neighbour (0 and
    the horizon at the ends) per step, after ``tau_bounds = (lo, hi)`` ([K] or [B, K]), so the existing waypoints of a row stay
    strictly ordered inside the horizon whatever the rule proposed.  Under "Nesterov" the tau point is the look-ahead
    ``taus + mu m_tau`` passed through the same projection against ``taus``.  A row frozen for the step (``skip_unconverged``) keeps
    its times and their moments bit for bit.  The clamp does NOT correct the moments when it binds: a velocity or first moment keeps
    pushing against the window until the gradient turns.  ``taus`` are the current times, ``tau_grad`` the last gradient, ``tau0``
    the demonstrated times (also the reference of the prior); ``step()`` keeps returning (loss, grad).  It combines with the five
    rules and per-row rule lists, ``interplation_level=2``, ``waypoint_weights`` / ``n_waypoints`` / ``pad_demonstrations`` (an absent
    waypoint has gradient +0 and is never read or moved), ``warm_start``, ``skip_unconverged``, ``trace`` and
    ``true_loss_print_flag`` (the second evaluation runs at ``taus``).  Refused with ``LfsdError``: ``loss_fn``, ``method="LM"`` (the
    first-order update of the times does not run beside the LM step: ``lm_taus`` below takes the joint step), ``stop_rule`` (its gather of ``taus`` runs only when the
    set shrinks), initial times that are not strictly increasing inside [0, horizon] among the existing waypoints, and
    ``tau_learning_rate=None``.

    ``lm_taus`` (default ``False`` = every learner makes the launches it made; ``method="LM"`` only): the waypoint times become unknowns of
    the Levenberg-Marquardt step.  A time enters the residuals of its own waypoint only, so the Gauss-Newton matrix in (theta, tau) is an
    arrow: H, a border ``c_k = w_k J_k^T t_k`` and a diagonal ``d_k = w_k t_k^T t_k`` with t_k the interface rows of the slope xdot(tau_k).
    One step: the evaluation at (``theta_trial``, ``tau_trial``) with the sensitivity grids; ``lfsd_normal_matrix``;
    ``lfsd_waypoint_time_grad`` without a prior; ``lfsd_time_normal_blocks`` (C, d); in grouped mode ``lfsd_group_reduce``;
    ``lfsd_lm_step_times`` -- accept / reject over the whole point, the times eliminated per waypoint, the p x p solve, the times by
    back-substitution (``group_size = demos_per_seed``, ``row_ok`` from ``skip_unconverged``); ``lfsd_tau_project`` of ``tau_trial``
    against the accepted times (``tau_max_shift``, ``tau_bounds``).  ``taus`` are the ACCEPTED times, ``tau_trial`` the next ones,
    ``tau_grad`` the last time gradient, ``tau0`` the demonstrated times, ``time_blocks`` the pair (C [B, K, p], d [B, K]) at the accepted
    point; ``step()`` returns loss and gradient at the trial point as LM does.  It combines with independent and grouped mode,
    ``waypoint_weights`` / ``n_waypoints``, ``interplation_level=2``, ``warm_start``, ``skip_unconverged`` and ``trace``.  Refused with
    ``LfsdError``: without ``method="LM"``; with ``learn_taus``; ``tau_learning_rate`` / ``tau_method`` / ``tau_prior`` (a prior term is not
    part of this step's objective); what ``method="LM"`` refuses; ``stop_rule``; initial times that are not strictly increasing.  A row
    needs more residuals than unknowns (K n_iface > p + K) for its times to be identified.
    """

    def __init__(self, oc, ini_state, horizon, taus, waypoints, interface_idx, theta0, method="Vanilla",
                 learning_rate=1e-2, mu=0.9, beta_1=0.9, beta_2=0.999, epsilon=1e-8, proj_lo=None, consts=None,
                 mode="independent", process_group=None, true_loss_print_flag=False, warm_start=False,
                 skip_unconverged=None, stop_rule=None, interplation_level=1, loss_fn=None, grad_scale=1.0, trace=None,
                 lm_lambda0=1e-2, lm_down=1.0 / 3.0, lm_up=2.0, lm_min=1e-8, lm_max=1e8, demos_per_seed=None,
                 waypoint_weights=None, n_waypoints=None, learn_taus=False, tau_learning_rate=None, tau_method=None,
                 tau_max_shift=0.25, tau_bounds=None, tau_prior=0.0, lm_taus=False):
        self.oc, self.method, self.lr, self.mu = oc, method, learning_rate, mu
        self._tau = None              # state of the learnable waypoint times (learn_taus), None: the times are data
        self._tau_pt = None           # the times the next evaluation runs at when they differ from `taus` (the look-ahead point)
        self._lmt = None              # state of the times inside the Levenberg-Marquardt step (lm_taus)
        self.tau_grad = None
        if lm_taus:
            if learn_taus:
                raise LfsdError("learn_taus and lm_taus are two ways of learning the times (a first-order rule beside theta's update, or "
                                "inside the joint step of method='LM'): give one")
            if method != "LM":
                raise LfsdError("lm_taus puts the waypoint times into the Levenberg-Marquardt step: method='LM' only (got %r; "
                                "learn_taus=True learns them under the first-order rules)" % (method,))
            given = [nm for nm, v in (("tau_learning_rate", tau_learning_rate), ("tau_method", tau_method)) if v is not None]
            if not (isinstance(tau_prior, (int, float)) and float(tau_prior) == 0.0):
                given.append("tau_prior")
            if given:
                raise LfsdError("%s with lm_taus: the joint step has no learning rate or rule of its own for the times, and a prior "
                                "term is not part of this step's objective (the sum of squares of the waypoint residuals)" % ", ".join(given))
            if stop_rule is not None:
                raise LfsdError("lm_taus does not combine with stop_rule yet: the dense batch gathers taus only when the set of "
                                "seeds shrinks, moving times would need it every step")
        if learn_taus:
            if loss_fn is not None:
                raise LfsdError("learn_taus differentiates the fused waypoint loss in its times: a loss_fn samples taus on its own")
            if method == "LM":
                raise LfsdError("learn_taus with method='LM': the first-order update of the times does not run beside the LM step; "
                                "lm_taus=True takes the joint Gauss-Newton step over theta and the times (DESIGN.md section 18), or use "
                                "one of the five first-order rules")
            if stop_rule is not None:
                raise LfsdError("learn_taus does not combine with stop_rule yet: the dense batch gathers taus only when the set of "
                                "seeds shrinks, moving times would need it every step")
            if tau_learning_rate is None:
                raise LfsdError("learn_taus=True needs tau_learning_rate: times and parameters have different units, there is no "
                                "default step")
        if waypoint_weights is not None and n_waypoints is not None:
            raise LfsdError("waypoint_weights and n_waypoints are two spellings of one array (n_waypoints: weight 1 below the count, 0 "
                            "from it on): give one")
        if loss_fn is not None and (waypoint_weights is not None or n_waypoints is not None):
            raise LfsdError("waypoint_weights / n_waypoints weigh the fused loss: a loss_fn does its own weighting")
        self.demos_per_seed = self.n_groups = None
        if demos_per_seed is not None and mode != "grouped":
            raise LfsdError("demos_per_seed belongs to mode='grouped' (mode=%r gives every row %s)"
                            % (mode, "the one theta" if mode == "shared" else "its own theta and one demonstration"))
        if mode == "grouped":
            D = demos_per_seed
            if D is None or isinstance(D, bool) or int(D) != D or int(D) <= 0:
                raise LfsdError("mode='grouped' needs demos_per_seed, a positive number of demonstrations per seed (got %r)" % (D,))
            self.demos_per_seed = int(D)
            if stop_rule is not None:
                raise LfsdError("stop_rule does not combine with mode='grouped' yet: the dense batch would have to keep whole groups "
                                "together (bookkeeping per group)")
            if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
                raise LfsdError("mode='grouped' issues no all-reduce: a process_group or an initialised torch.distributed would be "
                                "ignored silently (every rank learns its own groups)")
            if self._per_row(true_loss_print_flag) is not None:
                raise LfsdError("true_loss_print_flag per group: mode='grouped' takes a scalar flag (the second evaluation is reduced "
                                "for every group or for none)")
        if loss_fn is not None and not callable(loss_fn):
            raise LfsdError("loss_fn must be callable: loss_fn(x_tau [B,K,n], u_tau [B,K,m]) -> loss [B]")
        if loss_fn is not None and stop_rule is not None:
            raise LfsdError("loss_fn does not combine with stop_rule yet: the dense batch of the seeds still learning would have to "
                            "hand loss_fn its row ids")
        self.loss_fn, self.grad_scale = loss_fn, float(grad_scale)
        if interplation_level not in (1, 2):
            raise LfsdError("interplation_level must be 1 (linear) or 2 (cubic), got %r" % (interplation_level,))
        self.interplation_level = interplation_level
        self.b1, self.b2, self.eps = beta_1, beta_2, epsilon
        for mth in (list(method) if isinstance(method, (list, tuple, np.ndarray)) else [method]):
            if not isinstance(mth, str) or mth not in runtime.OPT_METHODS:
                raise Exception("Wrong optimization method type!")
        self._lm = None
        if not isinstance(method, str) and "LM" in list(method):
            raise LfsdError("method 'LM' in a per-row method list: the rows path carries the five first-order rules only "
                            "(lfsd_optimizer_step_rows); give method='LM' for the whole batch")
        if method == "LM":
            if loss_fn is not None:
                raise LfsdError("method='LM' needs the fused waypoint loss: a general loss_fn is not a sum of squares, so J^T J is not "
                                "a model of it")
            if mode not in ("independent", "grouped"):
                raise LfsdError("method='LM' keeps a damping and an accepted point per seed: mode='independent' (or 'grouped') only")
            if interface_idx is None:
                raise LfsdError("method='LM' needs interface_idx: with the interface function compiled into the library the Jacobian "
                                "of the residuals would need the generated dg/dx")
            hp = dict(lambda0=float(lm_lambda0), down=float(lm_down), up=float(lm_up), lo=float(lm_min), hi=float(lm_max))
            if not (0 < hp["down"] <= 1 and hp["up"] >= 1 and 0 < hp["lo"] <= hp["hi"] and hp["lo"] <= hp["lambda0"] <= hp["hi"]):
                raise LfsdError("method='LM' needs 0 < lm_down <= 1 <= lm_up and 0 < lm_min <= lm_lambda0 <= lm_max (got %s)" % hp)
            self._lm = hp
        self.mode, self.pg = mode, process_group
        self.lib = oc.compile()
        if mode == "grouped":
            ini_state, horizon, taus, waypoints = self._tile_demonstrations(ini_state, horizon, taus, waypoints, theta0)
        x0 = oc._t(ini_state)
        self.x0 = x0.unsqueeze(0) if x0.dim() == 1 else x0
        B = self.B = self.x0.shape[0]
        p = self.lib.n_auxvar
        hz = oc._t(horizon)
        self.hz = hz.expand(B).contiguous() if hz.dim() == 0 else hz
        tt = oc._t(taus)
        self.taus = tt.unsqueeze(0).expand(B, -1).contiguous() if tt.dim() == 1 else tt
        if loss_fn is not None and waypoints is None:      # (a user-written loss keeps its own targets)
            self.wps, self.iface, self.wts = None, None, None
            oc.check_time_range(self.taus, self.hz)
        else:
            wp = oc._t(waypoints)
            self.wps = wp.unsqueeze(0).expand(B, -1, -1).contiguous() if wp.dim() == 2 else wp
            self.iface = None if interface_idx is None else torch.as_tensor(list(interface_idx), dtype=torch.int32, device=self.x0.device)
            self.wts = self._init_weights(waypoint_weights, n_waypoints)
            oc.check_waypoints(self.taus, self.hz, interface_idx, self.wts)
        th = oc._t(theta0)
        th = th.unsqueeze(0) if th.dim() == 1 else th
        if mode == "shared":
            assert th.shape[0] == 1, "shared mode keeps a single parameter vector"
            self.theta = th.clone()
        elif mode == "grouped":
            G = self.n_groups
            if th.dim() != 2 or th.shape[0] not in (1, G) or th.shape[1] != p:
                raise LfsdError("theta0 has shape %s for %d groups of %d demonstrations: [p], [1, p] or [G, p] with p = %d"
                                % (tuple(th.shape), G, self.demos_per_seed, p))
            self.theta = th.expand(G, p).contiguous().clone()
            dev = self.x0.device
            # row -> its group, built once: lfsd_gather_rows expands the evaluation point [G, p] to the rows [B, p]
            self._group_of_row = (torch.arange(B, dtype=torch.int32, device=dev) // self.demos_per_seed).contiguous()
            self._theta_rows = torch.empty((B, p), dtype=self.theta.dtype, device=dev)
            self._grp_out = None
            self.row_loss = self.row_grad = self.n_ok = None
        else:
            self.theta = th.expand(B, p).contiguous().clone()
        self.consts = consts if consts is not None else oc.consts_tensor()
        z = lambda: torch.zeros_like(self.theta)
        self.m, self.v, self.vhat = z(), z(), z()
        lo = torch.full((p,), -float("inf"), dtype=torch.float64)
        for k, val in (proj_lo or {0: 1e-8}).items():      # examples: current_parameter[0] = fmax(., 1e-8)
            lo[k] = val
        self.proj_lo = lo.to(device=self.x0.device, dtype=self.theta.dtype)
        self.iter_idx = 0
        self.true_loss = true_loss_print_flag
        self._init_rows(method, learning_rate, mu, beta_1, beta_2, epsilon, true_loss_print_flag)
        if self._lm is not None:
            if self._rows_path:
                raise LfsdError("method='LM' with a per-row argument: the rows path carries the five first-order rules only")
            if p > 16:
                raise LfsdError("method='LM' factors a p x p matrix per lane: n_auxvar = %d > 16" % p)
            th, dev = self.theta, self.theta.device
            R = th.shape[0]                                   # rows of parameters: B, or the groups of mode='grouped'
            self.theta_trial = th.clone()                     # the point step() evaluates next (theta: the accepted point)
            self._lm.update(loss=torch.full((R,), float("inf"), dtype=th.dtype, device=dev), grad=torch.zeros_like(th),
                            H=torch.zeros((R, p, p), dtype=th.dtype, device=dev),
                            lam=torch.full((R,), self._lm["lambda0"], dtype=th.dtype, device=dev),
                            accepted=torch.zeros(R, dtype=torch.int32, device=dev))
            self._H_t = self._H_full = None
        self._init_trace(trace)
        self.tau0 = self.taus
        if learn_taus:
            self._init_taus(tau_learning_rate, tau_method, tau_max_shift, tau_bounds, tau_prior)
        if lm_taus:
            self._init_lm_taus(tau_max_shift, tau_bounds)
        # warm_start: start every OC solve from the previous iteration's controls (theta moves little per step).
        # The reference cold-starts IPOPT every time; the converged KKT point is the same, only the path to it is shorter.
        self.warm_start = warm_start
        self.skip_unconverged = (mode in ("shared", "grouped")) if skip_unconverged is None else bool(skip_unconverged)
        self.count_unconverged = True      # one small device->host read per step; switch off inside timed loops
        self.n_unconverged = 0
        self.n_bad_device = None
        self.event_hook = None
        self._ok = None
        self._ws = None
        self._sol = None
        self._aux = None
        self._Z = None
        self._stop = None
        if stop_rule is not None:
            if mode != "independent":
                raise LfsdError("stop_rule is a per-seed rule: mode='independent' only (shared mode keeps one theta for all)")
            unknown = set(stop_rule) - {"loss", "grad_norm"}
            if unknown or not {"loss", "grad_norm"} <= set(stop_rule):
                raise LfsdError("stop_rule takes exactly the keys 'loss' and 'grad_norm' (got %s)" % sorted(stop_rule))
            dev, i32 = self.x0.device, torch.int32
            self._stop = dict(loss=float(stop_rule["loss"]), grad_norm=float(stop_rule["grad_norm"]))
            self._active = torch.ones(B, dtype=i32, device=dev)
            self._stop_iter = torch.zeros(B, dtype=i32, device=dev)
            self._rows = [torch.arange(B, dtype=i32, device=dev), torch.empty(B, dtype=i32, device=dev)]      # ping-pong
            self._cur = 0
            self._pos = torch.empty(B, dtype=i32, device=dev)
            self._n_out = torch.zeros(1, dtype=i32, device=dev)
            self._dense = None           # dense copies of the per-row inputs, allocated when the first seed stops
            self._regather = False
            self._full = None            # the full-size solver buffers (leading slices of them hold the dense batch)
            self._prev = None            # (controls, status) of the previous solve of the rows now active, dense
            self._loss_full = self._grad_full = None
        self.n_active = B

    # ---- waypoint weights and ragged demonstrations (ABI 16) ----------------------------------------------------------------
    def _init_weights(self, weights, counts):
        """[B, K] weights in the dtype of ``taus`` on the device, or None when neither argument is given (the unweighted launches).
        Accepted in the shapes ``taus`` is: [K], [B, K], in grouped mode [D, K] tiled over the seeds; ``counts`` (n_waypoints):
        integers, a scalar, [B] or [D].  Checked here, once: finite and non-negative; counts inside [0, K]."""
        if weights is None and counts is None:
            return None
        B, K = self.taus.shape
        D = self.demos_per_seed
        lead = (B,) if D is None else (B, D)
        tile = lambda t: t if t.shape[0] == B else t.repeat((B // D,) + (1,) * (t.dim() - 1))
        if counts is not None:
            c = counts.detach().cpu() if isinstance(counts, torch.Tensor) else torch.as_tensor(np.asarray(counts))
            if c.dtype == torch.bool or c.is_floating_point() and not bool((c == c.round()).all()):
                raise LfsdError("n_waypoints counts waypoints: integers (got %r)" % (counts,))
            c = c.to(torch.int64)
            if c.dim() == 0:
                c = c.expand(B)
            elif c.dim() == 1 and c.shape[0] in lead:
                c = tile(c)
            else:
                raise LfsdError("n_waypoints has shape %s: a scalar or one count per row, leading dimension in %s" % (tuple(c.shape), lead))
            if bool((c < 0).any()) or bool((c > K).any()):
                raise LfsdError("n_waypoints outside [0, K = %d]: %s" % (K, c.tolist()))
            w = (torch.arange(K).unsqueeze(0) < c.unsqueeze(1)).to(torch.float64)
        else:
            w = weights.detach().double().cpu() if isinstance(weights, torch.Tensor) else torch.as_tensor(np.asarray(weights, dtype=np.float64))
            if w.dim() == 1 and w.shape[0] == K:
                w = w.unsqueeze(0).expand(B, K)
            elif w.dim() == 2 and w.shape[1] == K and w.shape[0] in lead:
                w = tile(w)
            else:
                raise LfsdError("waypoint_weights has shape %s: [K] or [rows, K] with K = %d and rows in %s, as taus"
                                % (tuple(w.shape), K, lead))
            self.oc.check_weights(w)
        return w.to(device=self.taus.device, dtype=self.taus.dtype).contiguous()

    def _wkw(self, wts):
        """The keyword that carries the weights into auxSysSolverBatch; without weights the call is what it always was."""
        return {} if wts is None else dict(waypoint_weights=wts)

    # ---- learnable waypoint times (ABI 17) ---------------------------------------------------------------------------------
    def _check_tau_args(self, who, max_shift, bounds, prior=None):
        """What learn_taus and lm_taus share, checked once: ``tau_max_shift`` in (0, 0.5), the initial times strictly increasing among
        the existing waypoints, ``tau_bounds``; ``tau_prior`` of learn_taus in the place it always had among them.  Returns (c, lo [B, K]
        or None, hi [B, K] or None)."""
        B, K = self.taus.shape
        dt, dev = self.taus.dtype, self.taus.device
        c = float(max_shift)
        if not 0 < c < 0.5:
            raise LfsdError("tau_max_shift must lie in (0, 0.5): a time moves by at most that fraction of the gap to its neighbour "
                            "per step, so the order cannot invert (got %r)" % (c,))
        if prior is not None and not (np.isfinite(prior) and prior >= 0):
            raise LfsdError("tau_prior must be finite and non-negative (got %r)" % (prior,))
        # the initial times: strictly increasing inside [0, horizon] among the waypoints that exist (one host read, at set-up)
        t = self.taus.detach().double().cpu().numpy()
        hz = self.hz.detach().double().cpu().numpy()
        w = None if self.wts is None else self.wts.detach().cpu().numpy()
        for b in range(B):
            tb = t[b] if w is None else t[b][w[b] != 0]
            if tb.size and not (np.all(np.isfinite(tb)) and tb[0] >= 0 and tb[-1] <= hz[b] and np.all(np.diff(tb) > 0)):
                raise LfsdError("%s needs initial taus strictly increasing inside [0, horizon] among the existing waypoints "
                                "(row %d: %s, horizon %g)" % (who, b, tb.tolist(), hz[b]))
        lo = hi = None
        if bounds is not None:
            if not isinstance(bounds, (tuple, list)) or len(bounds) != 2:
                raise LfsdError("tau_bounds is (lo, hi), each [K] or [B, K]")
            both = []
            for nm, x in zip(("lo", "hi"), bounds):
                x = x.detach().double().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64))
                if x.dim() == 1 and x.shape[0] == K:
                    x = x.unsqueeze(0).expand(B, K)
                elif tuple(x.shape) != (B, K):
                    raise LfsdError("tau_bounds %s has shape %s: [K] or [B, K] = %s" % (nm, tuple(x.shape), (B, K)))
                if bool(torch.isnan(x).any()):
                    raise LfsdError("tau_bounds %s holds a NaN" % nm)
                both.append(x.to(device=dev, dtype=dt).contiguous())
            lo, hi = both
        return c, lo, hi

    def _init_taus(self, lr, method, max_shift, bounds, prior):
        """State of ``learn_taus``: the times become a [B, K] array of their own with optimizer moments, checked once, here."""
        B, K = self.taus.shape
        dt, dev = self.taus.dtype, self.taus.device
        if method is None:
            method = self.method if isinstance(self.method, str) else "Vanilla"
        if not isinstance(method, str) or method not in runtime.OPT_METHODS or method == "LM":
            raise LfsdError("tau_method is one of the five first-order rules (got %r)" % (method,))
        lr, prior = float(lr), float(prior)
        if not (np.isfinite(lr) and lr >= 0):
            raise LfsdError("tau_learning_rate must be finite and non-negative (got %r)" % (lr,))
        c, lo, hi = self._check_tau_args("learn_taus", max_shift, bounds, prior)
        self.tau0 = self.taus.clone()         # the demonstrated times: tau_ref of the prior
        self.taus = self.taus.clone()         # (the learner's own array: the caller's tensor is never written)
        z = lambda: torch.zeros((B, K), dtype=dt, device=dev)
        # (the rule's other hyper-parameters are the learner's; where those are given per row, the defaults)
        sc = lambda x, dflt: dflt if self._per_row(x) is not None else float(x)
        self._tau = dict(method=method, lr=lr, c=c, prior=prior, lo=lo, hi=hi, m=z(), v=z(), vhat=z(), start=z(),
                         mu=sc(self.mu, 0.9), b1=sc(self.b1, 0.9), b2=sc(self.b2, 0.999), eps=sc(self.eps, 1e-8))
        self.tau_grad = z()

    m_tau = property(lambda self: None if self._tau is None else self._tau["m"], doc="[B, K] first moment / velocity of the times")
    v_tau = property(lambda self: None if self._tau is None else self._tau["v"], doc="[B, K] second moment of the times")
    vhat_tau = property(lambda self: None if self._tau is None else self._tau["vhat"], doc="[B, K] AMSGrad maximum of the times")

    def _tau_eval_point(self):
        """The times the step evaluates at: ``taus``, or under Nesterov the look-ahead ``taus + mu m_tau`` (the velocity is the
        array lfsd_optimizer_step keeps it in) passed through lfsd_tau_project against ``taus``, so it is ordered too."""
        s = self._tau
        if s["method"] != "Nesterov":
            return None
        look = self.lib.lookahead(self.taus, s["m"], s["mu"])
        return self.lib.tau_project(self.taus, look, self.hz, s["c"], wp_weight=self.wts, tau_lo=s["lo"], tau_hi=s["hi"])

    def _time_inputs(self):
        """What the kernels of the waypoint times read of the evaluation just made, in the sweeps' dtype (at level 2 the curvature grid
        is in it): the cast, the state grid's curvature grid or None, the state grid, the horizons and the times in use."""
        sol, aux = self._sol, self._aux
        ad = aux["loss"].dtype
        cv = lambda t: None if t is None else t.to(ad).contiguous()
        curv = aux["curvature"][0] if aux.get("curvature") is not None else None
        taus = self.taus if self._tau_pt is None else self._tau_pt
        return cv, curv, cv(sol["state_grid"]), cv(self.hz), cv(taus)

    def _tau_gradient(self):
        """dLoss/dtau (no factor 2) of the evaluation just made, from its solved state grid: one launch (lfsd_waypoint_time_grad)."""
        s = self._tau
        if self.event_hook is not None:
            self.event_hook("tau_grad")
        cv, curv, X, hz, taus = self._time_inputs()
        consts = cv(self._sol["consts"]) if self.iface is None else None
        g = self.lib.waypoint_time_grad(X, hz, taus, cv(self.wps), self.iface, curv=curv, consts=consts, wp_weight=cv(self.wts),
                                        tau_ref=cv(self.tau0) if s["prior"] > 0 else None, tau_prior=s["prior"],
                                        out=self.tau_grad if X.dtype == self.tau_grad.dtype else None)
        self.tau_grad = g.to(self.taus.dtype)
        return self.tau_grad

    def _tau_update(self, dtau, row_active, iter_idx):
        """The update of the times: lfsd_optimizer_step on ``taus`` and its own moments (p = K, no projection), then
        lfsd_tau_project against the times the step started from.  Rows with row_active == 0 keep times and moments bit for bit."""
        s = self._tau
        if self.event_hook is not None:
            self.event_hook("tau_update")
        s["start"].copy_(self.taus)
        self.lib.optimizer_step(s["method"], self.taus, dtau, iter_idx, s["lr"], s["mu"], s["b1"], s["b2"], s["eps"],
                                m=s["m"], v=s["v"], vhat=s["vhat"], proj_lo=None, row_active=row_active)
        self.lib.tau_project(s["start"], self.taus, self.hz, s["c"], wp_weight=self.wts, tau_lo=s["lo"], tau_hi=s["hi"],
                             row_active=row_active)

    # ---- the times inside the Levenberg-Marquardt step (lm_taus, ABI 18) -------------------------------------------------------
    def _init_lm_taus(self, max_shift, bounds):
        """State of ``lm_taus``: ``taus`` becomes the learner's own array of ACCEPTED times beside ``tau_trial``, with the time
        gradient and the border / diagonal of the arrow matrix at the accepted point, per row."""
        c, lo, hi = self._check_tau_args("lm_taus", max_shift, bounds)
        B, K = self.taus.shape
        p = self.theta.shape[1]
        dt, dev = self.theta.dtype, self.taus.device
        z = lambda *s: torch.zeros(s, dtype=dt, device=dev)
        self.tau0 = self.taus.clone()
        self.taus = self.taus.clone()         # (the learner's own array: the caller's tensor is never written)
        self._lmt = dict(c=c, lo=lo, hi=hi, trial=self.taus.clone(), gtau=z(B, K), C=z(B, K, p), d=z(B, K),
                         ok=torch.zeros(B, dtype=torch.int32, device=dev), gtau_t=None, C_t=None, d_t=None)
        self.tau_grad = z(B, K)

    tau_trial = property(lambda self: None if self._lmt is None else self._lmt["trial"],
                         doc="[B, K] the times step() evaluates next (lm_taus; taus: the accepted times)")
    time_blocks = property(lambda self: None if self._lmt is None else (self._lmt["C"], self._lmt["d"]),
                           doc="(C [B, K, p], d [B, K]): coupling and time block of the Gauss-Newton matrix at the accepted point (lm_taus)")

    def _lm_time_terms(self):
        """Of the evaluation just made (in step(): at tau_trial): dLoss/dtau without a prior (lfsd_waypoint_time_grad) and the
        coupling / time blocks (lfsd_time_normal_blocks), in the sweeps' dtype, cast to theta's.  Two launches."""
        s, hook = self._lmt, self.event_hook
        cv, curv, X, hz, taus = self._time_inputs()
        wts = cv(self.wts)
        if hook is not None:
            hook("tau_grad")
        g = self.lib.waypoint_time_grad(X, hz, taus, cv(self.wps), self.iface, curv=curv, wp_weight=wts)
        if hook is not None:
            hook("time_blocks")
        C, d = self.lib.time_normal_blocks(X, hz, taus, self._aux["auxX_grid"], self.iface, curv=curv, wp_weight=wts)
        dt = self.theta.dtype
        s["gtau_t"], s["C_t"], s["d_t"] = g.to(dt), C.to(dt), d.to(dt)
        self.tau_grad = s["gtau_t"]

    # ---- per-row update rules (hyper-parameter sweeps in one batch) and device traces -------------------------------------
    @staticmethod
    def _per_row(x):
        """None for a scalar argument, else its values as a list."""
        if isinstance(x, torch.Tensor):
            return None if x.dim() == 0 else x.detach().cpu().tolist()
        if isinstance(x, np.ndarray):
            return None if x.ndim == 0 else x.tolist()
        if isinstance(x, (list, tuple)):
            return list(x)
        return None

    def _init_rows(self, method, learning_rate, mu, beta_1, beta_2, epsilon, true_loss):
        B, dev = (self.n_groups if self.mode == "grouped" else self.B), self.x0.device      # (rows of parameters)
        seqs = dict(method=list(method) if isinstance(method, (list, tuple, np.ndarray)) else None, learning_rate=self._per_row(learning_rate),
                    mu=self._per_row(mu), beta_1=self._per_row(beta_1), beta_2=self._per_row(beta_2), epsilon=self._per_row(epsilon),
                    true_loss_print_flag=self._per_row(true_loss))
        self._rows_path = any(v is not None for v in seqs.values())
        if not self._rows_path:
            return
        if self.mode == "shared":
            raise LfsdError("per-row %s: mode='shared' keeps one theta for all demonstrations (mode='independent' only)"
                            % ", ".join(k for k, v in seqs.items() if v is not None))
        for k, v in seqs.items():
            if v is not None and len(v) != B:
                raise LfsdError("%s has %d entries for a batch of %d %s" % (k, len(v), B, "groups" if self.mode == "grouped" else "rows"))
        full = lambda v, scalar: [scalar] * B if v is None else v
        methods = full(seqs["method"], method)
        codes = np.array([runtime.OPT_METHODS[mth] for mth in methods], dtype=np.int32)
        # assembled in fp64, cast once: the numbers lfsd_optimizer_step gets by casting its double arguments
        hyper = np.stack([np.asarray(full(seqs[k], sc), dtype=np.float64) for k, sc in
                          (("learning_rate", learning_rate), ("mu", mu), ("beta_1", beta_1), ("beta_2", beta_2),
                           ("epsilon", epsilon))], axis=1)
        self.method = list(methods)
        self._method_rows = torch.from_numpy(codes).to(dev)
        self._hyper = torch.from_numpy(hyper).to(device=dev, dtype=self.theta.dtype).contiguous()
        nesterov = codes == runtime.OPT_METHODS["Nesterov"]
        self._any_nesterov = bool(nesterov.any())
        flagged = nesterov & np.array([bool(f) for f in full(seqs["true_loss_print_flag"], true_loss)])
        self._true_rows = torch.from_numpy(flagged).to(dev) if flagged.any() else None

    def _init_trace(self, trace):
        self.loss_trace = self.grad_norm_trace = self.theta_trace = None
        self._trace_cap = None
        if trace is None:
            return
        if isinstance(trace, bool) or int(trace) != trace or int(trace) <= 0:
            raise LfsdError("trace is None or the capacity of the traces, a positive number of steps (got %r)" % (trace,))
        cap, th = int(trace), self.theta
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=th.dtype, device=th.device)
        self._trace_cap = cap
        self.loss_trace, self.grad_norm_trace = nan(th.shape[0], cap), nan(th.shape[0], cap)
        self.theta_trace = nan(th.shape[0], cap + 1, th.shape[1])
        self.theta_trace[:, 0] = th

    def _check_trace_room(self):
        if self._trace_cap is not None and self.iter_idx >= self._trace_cap:
            raise LfsdError("step %d does not fit the traces: trace=%d" % (self.iter_idx + 1, self._trace_cap))

    def _eval_point(self):
        """Where the update rules want loss and gradient: theta, or the Nesterov look-ahead point (QuadAlgorithm.py:478)."""
        if self._lm is not None:
            return self.theta_trial
        if not self._rows_path:
            return self.lib.lookahead(self.theta, self.m, self.mu) if self.method == "Nesterov" else self.theta
        if not self._any_nesterov:
            return self.theta
        return self.lib.lookahead_rows(self._method_rows, self._hyper, self.theta, self.m)

    def _update(self, grad, row_active, loss=None):
        if self._lmt is not None:     # the same over (theta, tau): lfsd_lm_step_times, then the proposed times are put in order
            s, t = self._lm, self._lmt
            D = self.demos_per_seed or 1
            row_ok = None if self._ok is None else self._ok.to(torch.int32)
            self.lib.lm_step_times(self.theta, s["loss"], s["grad"], s["H"], s["lam"], self.theta_trial, self.taus, t["trial"], t["gtau"],
                                   t["C"], t["d"], t["ok"], loss.contiguous(), grad.contiguous(), self._H_t, t["gtau_t"].contiguous(),
                                   t["C_t"].contiguous(), t["d_t"].contiguous(), group_size=D, lambda_down=s["down"], lambda_up=s["up"],
                                   lambda_min=s["lo"], lambda_max=s["hi"], row_ok=row_ok, wp_weight=self.wts, proj_lo=self.proj_lo,
                                   group_active=row_active, accepted=s["accepted"])
            rows = row_active if row_active is None or D == 1 else row_active.repeat_interleave(D).contiguous()
            self.lib.tau_project(self.taus, t["trial"], self.hz, t["c"], wp_weight=self.wts, tau_lo=t["lo"], tau_hi=t["hi"], row_active=rows)
        elif self._lm is not None:      # accept / reject the point just evaluated and solve for the next one (lfsd_lm_step)
            s = self._lm
            self.lib.lm_step(self.theta, s["loss"], s["grad"], s["H"], s["lam"], self.theta_trial, loss.contiguous(), grad.contiguous(),
                             self._H_t, lambda_down=s["down"], lambda_up=s["up"], lambda_min=s["lo"], lambda_max=s["hi"],
                             proj_lo=self.proj_lo, row_active=row_active, accepted=s["accepted"])
        elif not self._rows_path:
            self.lib.optimizer_step(self.method, self.theta, grad, self.iter_idx, self.lr, self.mu, self.b1, self.b2, self.eps,
                                    m=self.m, v=self.v, vhat=self.vhat, proj_lo=self.proj_lo, row_active=row_active)
        else:
            self.lib.optimizer_step_rows(self._method_rows, self._hyper, self.theta, grad, self.iter_idx, self.m, self.v, self.vhat,
                                         proj_lo=self.proj_lo, row_active=row_active)

    def _second_evaluation(self, evaluate, flag):
        """The evaluation at theta that flagged Nesterov rows take their loss and gradient from (QuadAlgorithm.py:487-492), run on
        the whole (active) batch.  Every OTHER row is left as its uniform learner leaves it, which has no second evaluation: the
        controls and status its next solve starts from, and its entry of the frozen-row mask, stay those of the first evaluation.
        `flag` [rows evaluated] bool.  Returns what `evaluate()` returns."""
        first, ok1 = self._start_state(), self._ok
        if first is not None:
            first = tuple(t.clone() for t in first)
        out = evaluate()
        if first is not None:
            for t, t1 in zip(self._start_state(), first):
                t.copy_(torch.where(flag.reshape((-1,) + (1,) * (t.dim() - 1)), t, t1))
        if ok1 is not None and self._ok is not None:
            self._ok = torch.where(flag, self._ok, ok1)
        return out

    def _append_trace(self, loss, grad, row_active):
        """After the update of iteration iter_idx - 1: what step() returns and theta after the projection."""
        if self._trace_cap is not None:
            self.lib.trace_append(self.iter_idx - 1, loss.contiguous(), grad.contiguous(), self.theta, loss_trace=self.loss_trace,
                                  gnorm_trace=self.grad_norm_trace, theta_trace=self.theta_trace, row_active=row_active)

    def _normal_matrix(self, aux, hz, taus, wts=None):
        """H = J^T J [rows, p, p] of the evaluation `aux` (sensitivity grids written), in the sweeps' dtype, cast to theta's.
        `wts`: the rows' waypoint weights (H = sum_k w_k J_k^T J_k), or None."""
        aX = aux["auxX_grid"]
        cv = lambda t: t.to(aX.dtype).contiguous()
        kw = {} if wts is None else dict(wp_weight=cv(wts))
        return self.lib.normal_matrix(cv(hz), cv(taus), aX, self.iface, **kw).to(self.theta.dtype)

    lm_lambda = property(lambda self: None if self._lm is None else self._lm["lam"], doc="[B] damping of every seed (method='LM')")
    lm_loss = property(lambda self: None if self._lm is None else self._lm["loss"],
                       doc="[B] loss at the accepted point, +inf before the first acceptance (method='LM')")
    lm_accepted = property(lambda self: None if self._lm is None else self._lm["accepted"] != 0,
                           doc="[B] bool: the seed accepted its trial point in the last step (method='LM')")
    normal_matrix = property(lambda self: None if self._lm is None else self._lm["H"],
                             doc="[B, p, p] Gauss-Newton matrix J^T J at the accepted point (method='LM'): small eigenvalues are "
                                 "directions of theta the waypoints do not pin down")

    @property
    def active(self):
        """[B] bool: seeds still learning (all of them without a stop rule)."""
        if self._stop is None:
            return torch.ones(self.B, dtype=torch.bool, device=self.x0.device)
        return self._active != 0

    @property
    def stop_iter(self):
        """[B] int32: outer iterations a stopped seed took (the reference loop's count), 0 while it is still learning."""
        if self._stop is None:
            return torch.zeros(self.B, dtype=torch.int32, device=self.x0.device)
        return self._stop_iter

    # ---- one evaluation: the rows being evaluated, their solve and their sweeps ------------------------------------------------
    def evaluate(self, theta):
        """(loss [B], grad [B,p]) of every trajectory at parameters theta ([B,p] or [1,p]).  mode='grouped': the group sums
        (loss [G], grad [G,p]) at theta [G,p] or [1,p]; any other shape is refused."""
        if self.mode == "grouped":
            G, p = self.theta.shape
            if not isinstance(theta, torch.Tensor) or theta.dim() != 2 or theta.shape[1] != p or theta.shape[0] not in (1, G) \
                    or theta.dtype != self.theta.dtype:
                raise LfsdError("mode='grouped' evaluates theta [%d, %d] (or [1, %d], expanded to the groups) of dtype %s, got %s"
                                % (G, p, p, self.theta.dtype, (tuple(theta.shape), theta.dtype) if isinstance(theta, torch.Tensor) else type(theta)))
            if theta.shape[0] != G:      # (the index row -> row // D reaches G - 1: the gather must find G rows)
                theta = theta.expand(G, p)
        return self._evaluate(theta, dense=False)

    def _start_state(self, dense=None):
        """(controls, status) the next solve of the rows now evaluated starts from (warm_start / skip_unconverged), or None."""
        if not (self.warm_start or self.skip_unconverged):
            return None
        if self._dense_now() if dense is None else dense:
            return self._prev
        return None if self._sol is None else (self._sol["control_grid"], self._sol["status"])

    def _dense_now(self):
        """A stop rule has stopped seeds: the solve and the sweeps run on the dense batch of the others."""
        return self._stop is not None and self.n_active < self.B

    def _rows_view(self, dense):
        """The rows being evaluated: their number, the per-row inputs, the (controls, status) their solve starts from and the buffers
        the solve and the sweeps write -- reused from step to step.  Full batch: the learner's own tensors and the outputs of its last
        evaluation.  Dense (after seeds have stopped): the leading n_active rows of the dense copies and of the full-size buffers."""
        start = self._start_state(dense)
        if not dense:
            taus = self.taus if self._tau_pt is None else self._tau_pt      # (learned times: their look-ahead or trial point)
            return dict(n=self.B, dense=False, x0=self.x0, hz=self.hz, taus=taus, wps=self.wps, wts=self.wts, consts=self.consts,
                        start=start, sol_out=self._sol_out(), aux_out=self._aux_out(), Z=self._Z)
        n, d, full = self.n_active, self._dense, self._full
        lead = lambda k, absent=None: d[k][:n] if k in d else absent
        return dict(n=n, dense=True, x0=lead("x0"), hz=lead("hz"), taus=lead("taus"), wps=lead("wps"), wts=lead("wts"),
                    consts=lead("consts", self.consts), start=None if start is None else tuple(t[:n] for t in start),
                    sol_out={k: t[:n] for k, t in full["sol"].items()}, aux_out={k: t[:n] for k, t in full["aux"].items()},
                    Z=full["Z"][:n])

    def _evaluate_view(self, view, theta):
        """(loss [n], grad [n,p]) of the rows of `view` at theta [n,p]: the solve, the two sweeps (fused loss, or the sensitivity grids
        and `loss_fn`), for method='LM' the Gauss-Newton matrix (and the time terms of lm_taus), the casts to theta's dtype, the mask
        of skip_unconverged."""
        oc, hook = self.oc, self.event_hook
        u_init = None
        if view["start"] is not None:
            prev, status = view["start"][0][:, :-1], view["start"][1]
            if self.warm_start:
                u_init = prev.contiguous()
            elif self.skip_unconverged:
                # a solve that ran out of iterations is continued from where it stopped instead of restarted (its parameters
                # did not move, a cold start would fail the same way); all others start from zero controls = cold start
                cont = (status == 3).reshape(-1, 1, 1)
                u_init = torch.where(cont & torch.isfinite(prev), prev, torch.zeros_like(prev)).contiguous()
        if hook is not None:
            hook("oc_solve")
        sol = oc.cocSolverBatch(view["x0"], view["hz"], theta, consts=view["consts"], u_init=u_init, workspace=self._ws,
                                out=view["sol_out"])
        self._ws = sol["workspace"]
        # a learner that freezes unconverged rows anyway does not pay for differentiating them (they are masked by their
        # status below): the diverged seeds of a fixed learning rate otherwise hold the Riccati launch 20x longer
        kw = dict(Z_grid=view["Z"], out=view["aux_out"], validate=False, skip_status=(3, 4) if self.skip_unconverged else None,
                  phase_hook=None if hook is None else (lambda nm: hook("aux_" + nm) if nm != "end" else None),
                  interplation_level=self.interplation_level)
        lm = self._lm is not None                        # (LM: the sensitivity grids are written too, J^T J is formed from them)
        if self.loss_fn is not None:
            aux = oc.auxSysSolverBatch(sol, want_grids=True, **kw)
        else:
            aux = oc.auxSysSolverBatch(sol, view["taus"], view["wps"], self.iface, want_grids=lm, **kw, **self._wkw(view["wts"]))
        if view["dense"]:
            self._sol_active, self._aux_active = sol, aux
            self._prev = (sol["control_grid"], sol["status"])
        else:
            self._sol, self._aux, self._Z = sol, aux, aux["Z_grid"]
        if self.loss_fn is not None:
            loss, grad = self._loss_fn_gradient(sol, aux, view)
        else:
            if lm:
                if hook is not None:
                    hook("normal_matrix")
                self._H_t = self._normal_matrix(aux, view["hz"], view["taus"], view["wts"])
                if self._lmt is not None:
                    self._lm_time_terms()
            loss, grad = aux["loss"].to(self.theta.dtype), aux["grad"].to(self.theta.dtype)
        if self.skip_unconverged:
            loss, grad = self.mask_unconverged(sol["status"], loss, grad, stats=aux.get("stats"))
        return loss, grad

    def _loss_fn_gradient(self, sol, aux, view):
        """(loss [n], grad [n,p]) of the user-written loss at the solution `sol` with the sensitivity grids of `aux` (class docstring)."""
        oc, lib, hook = self.oc, self.lib, self.event_hook
        if hook is not None:
            hook("loss_fn")
        hz, taus = view["hz"], view["taus"]
        if aux["curvature"] is not None:      # level 2: the curvature grids the sweeps fitted serve the sampling too
            sol = dict(sol, curvature=aux["curvature"])
        s = oc.sampleBatch(sol, taus, self.interplation_level, validate=False)
        with torch.enable_grad():
            x_tau = s["state"].detach().requires_grad_(True)
            u_tau = s["control"].detach().requires_grad_(True)
            loss = self.loss_fn(x_tau, u_tau)
            if not isinstance(loss, torch.Tensor) or tuple(loss.shape) != (view["n"],):
                raise LfsdError("loss_fn must return one loss per trajectory, a [%d] tensor (got %s)"
                                % (view["n"], tuple(loss.shape) if isinstance(loss, torch.Tensor) else type(loss)))
            rx, ru = torch.autograd.grad(loss.sum(), (x_tau, u_tau), allow_unused=True)
        aX, aU = aux["auxX_grid"], aux["auxU_grid"]
        ad = aX.dtype                               # (the sweeps' arithmetic: aux_dtype may differ from the solve's)
        cv = lambda t: t.to(ad).contiguous()
        rx = torch.zeros_like(x_tau) if rx is None else rx
        grad = lib.waypoint_vjp(cv(hz), cv(taus), cv(rx), aX, ru=None if ru is None else cv(ru),
                                auxU_grid=None if ru is None else aU)
        if self.grad_scale != 1.0:
            grad = grad * self.grad_scale
        # a row the sweeps skipped has NaN sensitivity grids and so a NaN gradient; its loss is NaN too, as the fused loss's
        # (its solve may have left finite state grids behind)
        status, loss = sol.get("status"), loss.detach()
        if status is not None:
            skipped = status == 4
            if self.skip_unconverged:
                skipped = skipped | (status == 3)
            loss = torch.where(skipped, torch.full_like(loss, float("nan")), loss)
        return loss.to(self.theta.dtype), grad.to(self.theta.dtype)

    def mask_unconverged(self, status, loss, grad, stats=None):
        """Rows whose OC solve neither converged (1) nor stalled at working precision (2), whose loss / gradient is
        not finite (parameters that have left the region where the problem is well posed, e.g. a cost weight driven
        negative), or whose sensitivity sweeps report an interval accepted above `aux_rtol` (the `stats` output of
        lfsd_aux_solve: refinement stopped gaining next to a conjugate point) are frozen for this step: ``self._ok`` masks them out of the update kernel; their gradient (and, in
        shared mode, their loss, which enters a sum) is zeroed."""
        ok = ((status == 1) | (status == 2)) & torch.isfinite(loss) & torch.isfinite(grad).all(dim=1)
        st = stats if stats is not None else (self._aux.get("stats") if self._aux is not None else None)
        if st is not None:      # ... or whose auxiliary sweeps accepted an interval above their tolerance (next to a conjugate point)
            ok = ok & ((st[:, 1] + st[:, 3]) == 0)
        self._ok = ok
        grad = torch.where(ok.unsqueeze(1), grad, torch.zeros_like(grad))
        if self.mode == "shared":
            loss = torch.where(ok, loss, torch.zeros_like(loss))
        return loss, grad

    def _sol_out(self):
        if self._sol is None:
            return None
        return {k: self._sol[k] for k in ("state_grid", "control_grid", "costate_grid", "cost", "iters", "status")}

    def _aux_out(self):
        if self._aux is None:
            return None
        return {k: self._aux[k] for k in ("loss", "grad", "stats")}

    def _evaluate(self, theta, dense=None):
        """(loss, grad) at theta, one entry per row of theta that is evaluated: theta is brought to the rows of the view (expanded;
        mode='grouped': lfsd_gather_rows over the groups' demonstrations; a stop rule's dense batch: lfsd_gather_rows of the seeds
        still learning, with the inputs that do not change gathered again only when the set shrank), the view is evaluated, and the
        mode reduces: mode='grouped' sums per group (lfsd_group_reduce: 0 plus the rows mask_unconverged left ok, ascending; with
        method='LM' the group's H too) and returns the sums [G]; the dense batch returns its [n_active] rows -- what the stop test
        reads -- after scattering them into the full-size ``_loss_full`` / ``_grad_full`` (and H).  `dense`: None = as the learner
        stands, False = the full batch whatever has stopped (``evaluate()``)."""
        lib, B = self.lib, self.B
        dense = self._dense_now() if dense is None else dense
        self._ok = None
        if self.mode == "grouped":
            th = lib.gather_rows(self._group_of_row, theta.contiguous(), self._theta_rows, B)
        elif dense:
            n, rows, d = self.n_active, self._rows[self._cur], self._dense
            lib.gather_rows(rows, theta, d["theta"], n)
            if self._regather:               # x0 / horizon / waypoints / per-trajectory constants: only when the set shrank
                for k, src in d["sources"].items():
                    lib.gather_rows(rows, src, d[k], n)
                self._regather = False
            th = d["theta"][:n]
        else:
            th = theta if theta.shape[0] == B else theta.expand(B, -1).contiguous()
        loss, grad = self._evaluate_view(self._rows_view(dense), th)
        lm = self._lm is not None
        if self.mode == "grouped":
            self.row_loss, self.row_grad = loss, grad
            if self.event_hook is not None:
                self.event_hook("group_reduce")
            row_ok = None if self._ok is None else self._ok.to(torch.int32)
            H = self._H_t.contiguous() if lm else None
            if self._grp_out is None:
                G, p, dt, dev = self.n_groups, grad.shape[1], self.theta.dtype, self.theta.device
                new = lambda *shape: torch.empty(shape, dtype=dt, device=dev)
                self._grp_out = (new(G), new(G, p), None if H is None else new(G, p, p), torch.empty(G, dtype=torch.int32, device=dev))
            loss, grad, H_g, self.n_ok = lib.group_reduce(loss.contiguous(), grad.contiguous(), self.demos_per_seed, H=H, row_ok=row_ok,
                                                          out=self._grp_out)
            if H_g is not None:
                self._H_rows, self._H_t = self._H_t, H_g      # (what lfsd_lm_step reads: the group's J^T J)
        elif dense:
            if lm:      # H of the dense rows goes to its seeds' rows of the full-size matrix, as loss and gradient do
                self._H_t = lib.scatter_rows(rows, self._H_t.contiguous(), self._H_full, n)
            lib.scatter_rows(rows, loss.contiguous(), self._loss_full, n)
            lib.scatter_rows(rows, grad.contiguous(), self._grad_full, n)
        return loss, grad

    def _shared_sum(self, loss, grad, all_reduce):
        """mode='shared': (loss [1], grad [1,p]) summed over the demonstrations; with `all_reduce` also over the ranks of the process
        group, in one packed all-reduce with the number of demonstrations left out (``n_bad_device``)."""
        g, l = grad.sum(dim=0, keepdim=True), loss.sum().reshape(1)
        if not all_reduce:
            return l, g
        n_bad = (self.B - self._ok.sum()).to(g.dtype).reshape(1) if self._ok is not None else torch.zeros_like(l)
        if self.pg is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            buf = torch.cat([g.reshape(-1), l, n_bad])
            torch.distributed.all_reduce(buf, group=self.pg)              # RCCL over xGMI on the GPU
            g, l, n_bad = buf[:-2].reshape(1, -1), buf[-2:-1], buf[-1:]
        self.n_bad_device = n_bad                                         # (device tensor: read it outside timed loops)
        return l, g.contiguous()

    # ---- per-seed stop rule: the dense batch of the seeds still learning ------------------------------------------
    def _apply_stop_rule(self, loss, grad):
        """Stop test + compaction of the rows just evaluated (loss [n], grad [n,p], n = n_active), then the bookkeeping of a
        set that shrank.  The one host read of the rule is here."""
        lib, n, B = self.lib, self.n_active, self.B
        rows = self._rows[self._cur]
        elig = None if self._ok is None else self._ok.to(torch.int32)      # frozen this step: its gradient was zeroed, not small
        lib.stop_compact(loss, grad, self._stop["loss"], self._stop["grad_norm"], self.iter_idx - 1, self._rows[1 - self._cur],
                         self._pos, self._n_out, self._active, self._stop_iter, rows_in=None if n == B else rows[:n],
                         eligible=elig)
        n_new = int(self._n_out.item())
        if n_new == n:
            return
        if self._dense is None:          # the first seeds stop: from here on the solver buffers hold a dense batch
            self._loss_full, self._grad_full = loss.clone(), grad.clone()
            if self._lm is not None:
                self._H_full = self._H_t.clone()
            self._full = dict(sol=self._sol_out(), aux=self._aux_out(), Z=self._Z)
            src = dict(x0=self.x0, hz=self.hz, taus=self.taus, wps=self.wps)
            if self.consts is not None and self.consts.dim() == 2:
                src["consts"] = self.consts
            if self.wts is not None:      # (the weights are gathered with taus and waypoints when the set shrinks)
                src["wts"] = self.wts
            self._dense = {k: torch.empty_like(t) for k, t in src.items()}
            self._dense.update(theta=torch.empty_like(self.theta), sources=src)
            self._prev = (self._sol["control_grid"], self._sol["status"])
        if n_new > 0 and (self.warm_start or self.skip_unconverged):
            # a continued solve continues ITS OWN row: the survivors' controls / status move to their new positions
            u, st = self._prev
            carry = (torch.empty((n_new,) + tuple(u.shape[1:]), dtype=u.dtype, device=u.device),
                     torch.empty((n_new,), dtype=st.dtype, device=st.device))
            lib.gather_rows(self._pos, u[:n], carry[0], n_new)
            lib.gather_rows(self._pos, st[:n], carry[1], n_new)
            self._prev = carry
        else:
            self._prev = None
        self._cur, self.n_active, self._regather = 1 - self._cur, n_new, True

    # ---- several demonstrations per seed (mode='grouped') -----------------------------------------------------------------
    def _tile_demonstrations(self, ini_state, horizon, taus, waypoints, theta0):
        """The four per-row inputs with B = G * D rows (row g * D + d: demonstration d of group g).  Each may come per demonstration
        (leading dimension D: tiled over the groups), per row (B), or broadcast as in the other modes.  B is the largest leading
        dimension given, at least D and at least D times the rows of theta0."""
        oc, D = self.oc, self.demos_per_seed
        # (name, tensor, dimensions of ONE row's value)
        items = [("ini_state", oc._t(ini_state), 1), ("horizon", oc._t(horizon), 0), ("taus", oc._t(taus), 1),
                 ("waypoints", None if waypoints is None else oc._t(waypoints), 2)]
        th = oc._t(theta0)
        lead = [t.shape[0] for _, t, nd in items if t is not None and t.dim() == nd + 1]
        B = max(lead + [D, D * (th.shape[0] if th.dim() == 2 else 1)])
        if B % D != 0:
            raise LfsdError("a batch of %d rows is not a whole number of groups of demos_per_seed = %d" % (B, D))
        G = self.n_groups = B // D
        out = []
        for name, t, nd in items:
            if t is None or t.dim() == nd:                     # broadcast (the constructor expands it to the rows)
                out.append(t)
                continue
            if t.dim() != nd + 1 or t.shape[0] not in (D, B):
                raise LfsdError("%s has shape %s: per demonstration (%d rows), per row (%d = %d groups x %d) or one value for all"
                                % (name, tuple(t.shape), D, B, G, D))
            out.append(t if t.shape[0] == B else t.repeat((G,) + (1,) * nd).contiguous())
        if out[0].dim() == 1:                                  # (the batch size is read from ini_state)
            out[0] = out[0].unsqueeze(0).expand(B, -1).contiguous()
        return out

    # ---- one outer iteration, every mode ---------------------------------------------------------------------------------------
    def step(self):
        """One outer iteration; returns (loss, grad) evaluated where the update rule needs them: per seed [B] (with a stop rule a
        stopped seed keeps its last values), the sums [1] of mode='shared', the group sums [G] of mode='grouped'."""
        lib, hook, B, n = self.lib, self.event_hook, self.B, self.n_active
        if n == 0:                       # every seed has stopped: nothing is launched
            return self._loss_full, self._grad_full
        self._check_trace_room()
        shared, D = self.mode == "shared", self.demos_per_seed
        rows = self._rows[self._cur] if n < B else None
        full_size = lambda l, g: (l, g) if n == B else (self._loss_full, self._grad_full)
        # the evaluation point: theta, the look-ahead or the LM trial point; for learned times their look-ahead or trial times
        theta_eval = self._eval_point()
        if self._tau is not None:
            self._tau_pt = self._tau_eval_point()
        if self._lmt is not None:
            self._tau_pt = self._lmt["trial"]
        loss, grad = self._evaluate(theta_eval)
        if self._tau is not None:
            dtau = self._tau_gradient()
        self._tau_pt = None
        if hook is not None:
            hook("update")
        if shared:
            loss, grad = self._shared_sum(loss, grad, all_reduce=True)
        # the rows of theta the update leaves alone: seeds stopped as of the last test (one that stops in this step is updated)
        # and, under skip_unconverged, what mask_unconverged froze for this step -- a seed, or a group none of whose
        # demonstrations counted (mode='shared' has the one theta: frozen demonstrations are left out of its sums)
        row_active = None if n == B else self._active
        rows_ok = None if self._ok is None else self._ok.to(torch.int32)
        if rows_ok is not None:
            if self.mode == "grouped":
                row_active = (self.n_ok > 0).to(torch.int32)
            elif not shared:
                row_active = rows_ok if n == B else lib.scatter_rows(rows, rows_ok, self._active.clone(), n)
            if self.count_unconverged:   # (one device->host read; in shared mode of the count over all ranks)
                self.n_unconverged = int(round(self.n_bad_device.item())) if shared else int(n - self._ok.sum().item())
        loss_out, grad_out = full_size(loss, grad)
        self._update(grad_out, row_active, loss_out)
        if self._tau is not None:        # (the times are per row in every mode: a frozen demonstration keeps its own)
            self._tau_update(dtau, rows_ok, self.iter_idx)
        self.iter_idx += 1
        if hook is not None:
            hook("end")
        # QuadAlgorithm.py:487-492: Nesterov's true loss, a second evaluation at theta, reduced as the first
        if self._true_rows is not None if self._rows_path else (self.method == "Nesterov" and bool(self.true_loss)):
            if not self._rows_path:
                loss, grad = self._evaluate(self.theta)
                if shared:
                    loss, grad = self._shared_sum(loss, grad, all_reduce=False)
            else:       # flagged Nesterov rows (groups) only take it, the others are left as their uniform learner leaves them
                first = (loss.clone(), grad.clone())      # (the solver's buffers: the second evaluation writes them again)
                n_ok = self.n_ok.clone() if D else None
                flag = self._true_rows if n == B else self._true_rows[rows[:n].long()]
                l2, g2 = self._second_evaluation(lambda: self._evaluate(self.theta), flag.repeat_interleave(D) if D else flag)
                loss, grad = torch.where(flag, l2, first[0]), torch.where(flag.unsqueeze(1), g2, first[1])
                if D:
                    self.n_ok = torch.where(flag, self.n_ok, n_ok)
                if n < B:
                    lib.scatter_rows(rows, loss, self._loss_full, n)
                    lib.scatter_rows(rows, grad, self._grad_full, n)
            loss_out, grad_out = full_size(loss, grad)
        self._append_trace(loss_out, grad_out, None if n == B else self._active)      # (active as of the previous test)
        if self._stop is not None:
            self._apply_stop_rule(loss, grad)
            if self._loss_full is not None:
                return self._loss_full, self._grad_full
        return loss_out, grad_out
