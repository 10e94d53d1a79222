"""Mirror of the reference's quadrotor driver (lib/QuadAlgorithm.py + lib/QuadPara.py, QuadStates.py,
DemoSparse.py, ObsInfo.py) on top of the HIP path.

Same constructor, ``load_optimization_function(para_dict)``, ``run(...)`` and ``getloss_pos_corrections``;
the learning loop (QuadAlgorithm.py:231-257) runs on the device through ``CPDP.SparseDemoLearner``.
Plotting / animation (QuadAlgorithm.py:260-281, 354-451, 581-613) is UI and is not reproduced; ``run`` returns the
dictionary the reference saves to ``data/uav_results_random_*.mat`` (QuadAlgorithm.py:324-333) and writes it only if
``save_flag`` is set.

``run_comparison(para_list, ...)`` is the batched form of the reference's test/*_comparison.py scripts: every configuration a block
of rows of one learner, traces kept on the device.

Extension: ``run(..., initial_parameters=[B,7])`` learns B independent seeds in lock-step.  ``stop="all"`` (default) leaves the
loop when EVERY seed has passed the reference's stop test; ``stop="per_seed"`` gives every seed that test on its own
(QuadAlgorithm.py:239-257 as the reference runs it, one seed per run): a seed that passes is frozen and leaves the launches, the
loop ends when none is left; ``results['stop_iter']`` [B] is the number of iterations each seed took (0: still learning at
``iter_num``), and the traces stay rectangular -- a stopped seed's last entry is repeated.  ``sample_all=True`` adds the final
trajectories of all seeds, ``results['opt_state_traj_all']`` [B,101,n] and ``results['opt_control_traj_all']`` [B,101,m] (one batched
solve at every seed's final parameters, sampled on the device: ``COCSys.sampleBatch``); the reference's keys stay those of seed 0.
"""
import os
import time
from dataclasses import dataclass, field

import numpy as np
import torch

from . import CPDP, JinEnv
from .JinEnv import QuadStates  # noqa: F401  (lib/QuadStates.py)
from .symbolic import SX, vertcat


@dataclass
class QuadPara:
    """lib/QuadPara.py."""
    inertial_x: float = 1
    inertial_y: float = 1
    inertial_z: float = 1
    mass: float = 1
    l: float = 1
    c: float = 1

    def __init__(self, inertial_list, mass, l, c):
        self.inertial_x, self.inertial_y, self.inertial_z = inertial_list
        self.mass, self.l, self.c = mass, l, c


@dataclass
class DemoSparse:
    """lib/DemoSparse.py."""
    waypoints: list = field(default_factory=lambda: [[0, 0, 0], [0, 0, 0], [0, 0, 0]])
    time_list: list = field(default_factory=lambda: [1, 2, 3])
    time_horizon: float = 4


@dataclass
class ObsInfo:
    """lib/ObsInfo.py (only carried along; obstacles are plotted, never used by the algorithm)."""
    length: float = 1
    width: float = 1
    height: float = 1
    center: list = field(default_factory=lambda: [0, 0, 0])

    def __init__(self, center_pisition, size_list):
        self.center = center_pisition
        self.length, self.width, self.height = size_list


class QuadAlgorithm(object):
    def __init__(self, config_data, QuadParaInput, n_grid, device=None, dtype=torch.float32):
        self.QuadPara = QuadParaInput
        self.n_grid = n_grid
        self.space_limit_x = config_data["LAB_SPACE_LIMIT"]["LIMIT_X"]
        self.space_limit_y = config_data["LAB_SPACE_LIMIT"]["LIMIT_Y"]
        self.space_limit_z = config_data["LAB_SPACE_LIMIT"]["LIMIT_Z"]
        self.quad_average_speed = float(config_data["QUAD_AVERAGE_SPEED"])
        self.device, self.dtype = device, dtype
        self.library = None          # tests may bind a prebuilt library (oc.use_library)

    def settings(self, QuadDesiredStates):
        """QuadAlgorithm.py:74-130: environment, time-warped OC system, interface = position."""
        self.env = JinEnv.Quadrotor()
        Q = self.QuadPara
        self.env.initDyn(Jx=Q.inertial_x, Jy=Q.inertial_y, Jz=Q.inertial_z, mass=Q.mass, l=Q.l, c=Q.c)
        self.env.initCost_Polynomial(QuadDesiredStates, w_thrust=0.1)
        self.oc = CPDP.COCSys()
        beta = SX.sym('beta')
        self.oc.setAuxvarVariable(vertcat(beta, self.env.cost_auxvar))
        self.oc.setStateVariable(self.env.X)
        self.oc.setControlVariable(self.env.U)
        self.oc.setDyn(beta * self.env.f)
        self.oc.setPathCost(beta * self.env.path_cost)
        self.oc.setFinalCost(self.env.final_cost)
        self.oc.setIntegrator(self.n_grid)
        self.oc.sys_name = "quadrotor_poly_tw"
        if self.library is not None:
            self.oc.use_library(self.library)
        self.oc.setDevice(self.device, self.dtype)
        self.interface_pos_idx = [0, 1, 2]
        self.interface_ori_idx = [6, 7, 8, 9]
        if self.optimization_method_str not in ("Vanilla", "Nesterov", "Adam", "Nadam", "AMSGrad", "LM"):
            raise Exception("Wrong optimization method type!")

    def load_optimization_function(self, para_input):
        """QuadAlgorithm.py:133-191 (same dictionary keys).  Beyond the reference: ``{"method": "LM", "iter_num": ...}`` with the
        optional keys ``lm_lambda0``, ``lm_down``, ``lm_up``, ``lm_min``, ``lm_max`` of ``SparseDemoLearner`` (Levenberg-Marquardt has no
        learning rate: ``learning_rate`` may be left out)."""
        self.learning_rate = para_input.get("learning_rate", 0.0) if para_input["method"] == "LM" else para_input["learning_rate"]
        self.iter_num = para_input["iter_num"]
        self.optimization_method_str = para_input["method"]
        self.opt_kwargs = {}
        m = para_input["method"]
        if m == "Vanilla":
            pass
        elif m == "Nesterov":
            self.mu_momentum = para_input["mu"]
            self.actual_loss_print_nesterov_flag = para_input["true_loss_print_flag"]
            self.opt_kwargs = dict(mu=self.mu_momentum, true_loss_print_flag=self.actual_loss_print_nesterov_flag)
        elif m in ("Adam", "Nadam", "AMSGrad"):
            self.opt_kwargs = dict(beta_1=para_input["beta_1"], beta_2=para_input["beta_2"],
                                   epsilon=para_input["epsilon"])
        elif m == "LM":
            self.opt_kwargs = {k: para_input[k] for k in ("lm_lambda0", "lm_down", "lm_up", "lm_min", "lm_max") if k in para_input}
        else:
            raise Exception("Wrong optimization method type!")

    def run(self, QuadInitialCondition, QuadDesiredStates, SparseInput, ObsList=(), print_flag=False, save_flag=False,
            initial_parameters=None, save_dir=None, stop="all", sample_all=False, waypoint_weights=None, learn_taus=False,
            tau_learning_rate=None, tau_method=None, tau_max_shift=0.25, tau_bounds=None, tau_prior=0.0, lm_taus=False):
        """``waypoint_weights`` ([K], or [S, K] with S seeds; default None): handed to ``SparseDemoLearner`` -- a confidence per
        waypoint, zero removes it (CPDP.SparseDemoLearner).
        ``learn_taus=True, tau_learning_rate=...`` (and ``tau_method``, ``tau_max_shift``, ``tau_bounds``, ``tau_prior``; read only with ``learn_taus``): the waypoint
        times are learned beside the parameters (CPDP.SparseDemoLearner; times on the normalised horizon, as ``time_grid``); the
        results then hold ``'taus'`` [S, K], the learned times, and ``'tau_trace'``, one entry per iteration plus the start.  Not
        together with ``stop="per_seed"``.
        ``lm_taus=True`` with a Levenberg-Marquardt optimisation function (and ``tau_max_shift``, ``tau_bounds``): the joint step over
        parameters and times (CPDP.SparseDemoLearner); ``'taus'`` are then the accepted times."""
        tau_kwargs = dict(tau_learning_rate=tau_learning_rate, tau_method=tau_method, tau_max_shift=tau_max_shift,
                          tau_bounds=tau_bounds, tau_prior=tau_prior)
        if stop not in ("all", "per_seed"):
            raise ValueError("stop must be 'all' or 'per_seed'")
        t0 = time.time()
        self.ObsList = ObsList
        self.settings(QuadDesiredStates)
        self.ini_state = (list(QuadInitialCondition.position) + list(QuadInitialCondition.velocity) +
                          list(QuadInitialCondition.attitude_quaternion) + list(QuadInitialCondition.angular_velocity))
        # QuadAlgorithm.py:221-223: the reference normalises the horizon to 1 and the waypoint times with it
        self.time_horizon = 1.0
        self.time_list_sparse = np.array(SparseInput.time_list) / SparseInput.time_horizon
        self.waypoints = np.array(SparseInput.waypoints)
        theta0 = np.array([1, 0.1, 0.1, 0.1, 0.1, 0.1, -1], dtype=float) if initial_parameters is None else \
            np.asarray(initial_parameters, dtype=float)                    # QuadAlgorithm.py:235
        self.learner = CPDP.SparseDemoLearner(self.oc, self.ini_state if theta0.ndim == 1 else
                                              np.tile(self.ini_state, (theta0.shape[0], 1)),
                                              self.time_horizon, self.time_list_sparse, self.waypoints,
                                              self.interface_pos_idx, theta0, method=self.optimization_method_str,
                                              learning_rate=self.learning_rate, **self.opt_kwargs,
                                              **({} if waypoint_weights is None else dict(waypoint_weights=waypoint_weights)),
                                              **(dict(learn_taus=True, **tau_kwargs) if learn_taus else {}),
                                              **(dict(lm_taus=True, tau_max_shift=tau_max_shift, tau_bounds=tau_bounds) if lm_taus else {}),
                                              **(dict(stop_rule=dict(loss=0.9, grad_norm=0.05)) if stop == "per_seed" else {}))
        self.loss_trace, self.parameter_trace = [], [self.learner.theta.cpu().numpy().copy()]
        self.tau_trace = [self.learner.taus.cpu().numpy().copy()] if learn_taus or lm_taus else None
        loss, diff_loss_norm = 100.0, 100.0
        for j in range(self.iter_num):
            if (self.learner.n_active > 0) if stop == "per_seed" else ((loss > 0.9) and (diff_loss_norm > 0.05)):   # QuadAlgorithm.py:242
                l, g = self.learner.step()
                loss = float(l.max())                                       # every seed must pass the stop test
                diff_loss_norm = float(torch.linalg.norm(g, dim=1).max())
                self.loss_trace.append(l.cpu().numpy().copy())
                self.parameter_trace.append(self.learner.theta.cpu().numpy().copy())
                if learn_taus or lm_taus:
                    self.tau_trace.append(self.learner.taus.cpu().numpy().copy())
                if print_flag:
                    print('iter:', j, ', loss:', self.loss_trace[-1], ', loss gradient norm:', diff_loss_norm)
            else:
                if print_flag:
                    print("The loss is less than threshold, stop the iteration.")
                break
        horizon = self.time_horizon
        current_parameter = self.parameter_trace[-1][0]
        _, opt_sol = self.oc.cocSolver(self.ini_state, horizon, current_parameter)
        time_steps = np.linspace(0, horizon, num=100 + 1)                   # QuadAlgorithm.py:309
        opt_traj = opt_sol(time_steps)
        n, m = self.oc.n_state, self.oc.n_control
        results = {'parameter_trace': np.array(self.parameter_trace), 'loss_trace': np.array(self.loss_trace),
                   'learning_rate': self.learning_rate, 'waypoints': self.waypoints,
                   'time_grid': self.time_list_sparse, 'time_steps': time_steps,
                   'opt_state_traj': opt_traj[:, :n], 'opt_control_traj': opt_traj[:, n:n + m],
                   'horizon': horizon, 'T': self.time_horizon, 'seconds': time.time() - t0}
        if sample_all:      # the final trajectory of EVERY seed (lib/QuadAlgorithm.py:306-317 per seed): one batched solve + sampling
            th_all = np.asarray(self.parameter_trace[-1], dtype=np.float64)
            sol = self.oc.cocSolverBatch(np.tile(self.ini_state, (th_all.shape[0], 1)), horizon, th_all)
            smp = self.oc.sampleBatch(sol, time_steps)
            results['opt_state_traj_all'] = smp["state"].double().cpu().numpy()
            results['opt_control_traj_all'] = smp["control"].double().cpu().numpy()
        if stop == "per_seed":
            results['stop_iter'] = self.learner.stop_iter.cpu().numpy().copy()
        if learn_taus or lm_taus:
            results['taus'] = self.tau_trace[-1]
            results['tau_trace'] = np.array(self.tau_trace)
        if save_flag:
            import scipy.io as sio
            d = save_dir or os.path.join(os.getcwd(), 'data')
            os.makedirs(d, exist_ok=True)
            sio.savemat(os.path.join(d, 'uav_results_random_' + time.strftime("%Y%m%d%H%M%S") + '.mat'),
                        {'results': results})
        return results

    def run_comparison(self, para_list, QuadInitialCondition, QuadDesiredStates, SparseInput, initial_parameters=None,
                       waypoint_weights=None):
        """The comparison scripts of the reference (test/opt_methods_comparison.py, test/*_learning_rate_comparison.py: one
        ``load_optimization_function`` + ``run`` per configuration, the loss traces overlaid) as ONE batch.  ``para_list``: the
        dictionaries ``load_optimization_function`` takes, with equal ``iter_num`` (else ``ValueError``); ``initial_parameters``: one
        theta_0 [7] (default: the reference's) or S seeds [S, 7], given to every configuration.  One learner of
        ``len(para_list) x S`` rows (configuration-major), every row with its own update rule, hyper-parameters and the reference's
        stop test (``stop_rule=dict(loss=0.9, grad_norm=0.05)``: each of the reference's runs has its own), traces on the device
        (``trace=iter_num``); the loop reads one int per step, the number of rows still learning.  Returns a dictionary:
          ``loss_trace_comparison``  per configuration what ``run(..., stop="per_seed")`` leaves in ``loss_trace`` for it: [stop_iter]
                                     for one theta_0, [iters, S] for seeds (iters: the configuration's slowest seed; a stopped seed's
                                     last entry is repeated, as ``run`` does);
          ``label_list``             the method names when the methods differ, else ``str(learning_rate)`` -- the scripts' labels;
          ``parameter_trace``        per configuration [stop_iter + 1, 7] or [iters + 1, S, 7];
          ``stop_iter``              per configuration the iterations it took, an int or [S] (0: still learning at ``iter_num``).
        ``waypoint_weights`` ([K], default None): a weight per waypoint for every row, handed to ``SparseDemoLearner``.
        Plotting stays with the caller (``plot_opt_method_comparison`` is UI)."""
        para_list = list(para_list)
        if not para_list:
            raise ValueError("run_comparison needs at least one configuration")
        if len({int(para["iter_num"]) for para in para_list}) != 1:
            raise ValueError("the configurations of one comparison share iter_num (got %s)" % [para["iter_num"] for para in para_list])
        C = len(para_list)
        rows = dict(method=[], learning_rate=[], mu=[], beta_1=[], beta_2=[], epsilon=[], true_loss_print_flag=[])
        for para in para_list:
            self.load_optimization_function(para)                 # (validates the dictionary as the reference does)
            kw = dict(dict(mu=0.9, beta_1=0.9, beta_2=0.999, epsilon=1e-8, true_loss_print_flag=False), **self.opt_kwargs)
            for k in rows:
                rows[k].append(dict(kw, method=self.optimization_method_str, learning_rate=self.learning_rate)[k])
        self.settings(QuadDesiredStates)
        self.ini_state = (list(QuadInitialCondition.position) + list(QuadInitialCondition.velocity) +
                          list(QuadInitialCondition.attitude_quaternion) + list(QuadInitialCondition.angular_velocity))
        self.time_horizon = 1.0                                    # QuadAlgorithm.py:221-223
        self.time_list_sparse = np.array(SparseInput.time_list) / SparseInput.time_horizon
        self.waypoints = np.array(SparseInput.waypoints)
        theta0 = np.array([1, 0.1, 0.1, 0.1, 0.1, 0.1, -1], dtype=float) if initial_parameters is None else \
            np.asarray(initial_parameters, dtype=float)
        single = theta0.ndim == 1
        seeds = theta0.reshape(-1, theta0.shape[-1])
        S, K = seeds.shape[0], self.iter_num
        per_row = {k: [v for v in vals for _ in range(S)] for k, vals in rows.items()}
        self.learner = CPDP.SparseDemoLearner(self.oc, np.tile(self.ini_state, (C * S, 1)), self.time_horizon, self.time_list_sparse,
                                              self.waypoints, self.interface_pos_idx, np.tile(seeds, (C, 1)),
                                              stop_rule=dict(loss=0.9, grad_norm=0.05), trace=K, **per_row,
                                              **({} if waypoint_weights is None else dict(waypoint_weights=waypoint_weights)))
        for _ in range(K):
            if self.learner.n_active == 0:
                break
            self.learner.step()
        stop = self.learner.stop_iter.cpu().numpy().reshape(C, S)
        loss = self.learner.loss_trace.cpu().numpy().reshape(C, S, K)
        theta = self.learner.theta_trace.cpu().numpy().reshape(C, S, K + 1, -1)
        took = np.where(stop == 0, K, stop)                        # entries a row's traces hold
        loss_cmp, par_cmp = [], []
        for i in range(C):
            n = int(took[i].max())
            l, th = loss[i, :, :n].copy(), theta[i, :, :n + 1].copy()
            for s_ in range(S):                                    # rectangular, as run(): a stopped seed's last entry repeated
                l[s_, took[i, s_]:] = l[s_, took[i, s_] - 1]
                th[s_, took[i, s_] + 1:] = th[s_, took[i, s_]]
            loss_cmp.append(l[0] if single else l.T.copy())
            par_cmp.append(th[0] if single else th.transpose(1, 0, 2).copy())
        methods = rows["method"]
        labels = list(methods) if len(set(methods)) > 1 else [str(lr) for lr in rows["learning_rate"]]
        self.loss_trace_comparison, self.label_list = loss_cmp, labels
        return {'loss_trace_comparison': loss_cmp, 'label_list': labels, 'parameter_trace': par_cmp,
                'stop_iter': [int(stop[i, 0]) if single else stop[i].copy() for i in range(C)]}

    def getloss_pos_corrections(self, time_grid, target_waypoints, opt_sol, auxsys_sol):
        """QuadAlgorithm.py:616-639 on host objects returned by cocSolver / auxSysSolver (same formula the kernel fuses)."""
        n, p = self.oc.n_state, self.oc.n_auxvar
        loss, diff_loss = 0.0, np.zeros(p)
        for k, t in enumerate(time_grid):
            target = np.asarray(target_waypoints[k])[0:3]
            cur = opt_sol(t)[0:n][0:3]
            loss += np.linalg.norm(target - cur) ** 2
            dxpos_dp = auxsys_sol(t)[0:n * p].reshape((n, p))
            diff_loss += (cur - target) @ dxpos_dp[0:3]
        return loss, diff_loss
