"""Krylov solver facade with the reference's KspSolver interface.

Mirrors ``src/solver/ksp_solver.py:6-19`` (``KspSolver(KSP)``: ``createSolver(mat, comm)``, then
``solver(b, x)`` == ``KSP.__call__`` == solve).  PETSc's KSP/PC objects become one C-ABI call,
``pyn_solve`` (device-resident Jacobi-PCG / GMRES).  Options follow PETSc's names:
``-ksp_type cg|gmres|preonly  -pc_type jacobi|none|lu  -ksp_rtol -ksp_atol -ksp_divtol
-ksp_max_it -ksp_gmres_restart -ksp_norm_type preconditioned|unpreconditioned|natural
-ksp_gmres_modifiedgramschmidt -ksp_gmres_cgs_refinement_type refine_never|refine_ifneeded|refine_always``
(GMRES orthogonalisation; default as in PETSc: classical Gram-Schmidt without refinement).
``-pynama_mat_free`` (not a PETSc name; PETSc's analogue is KSPSetOperators(Amat = MATSHELL, Pmat = assembled)): CG multiplies
with the matrix-free form of the operator when the matrix carries one (``Mat.K`` on structured Q1 hex meshes) -- the
assembled matrix then only supplies the Jacobi diagonal and the exit check; the library verifies that both agree on ``b``
before it iterates.  Without the option the choice is automatic: CG (and the symmetric ``preonly`` substitute) take the shell
whenever the matrix carries one -- 4 x the iteration rate of the assembled product at 128^3 -- and go back to the assembled
product, with a warning, if the library finds that the two differ; ``-pynama_mat_free 0`` keeps the assembled product.
On second-order (ngl 3) structured meshes of affine cells ``Mat.K`` carries the shell only with ``-pynama_mat_free_ngl3``
(opt-in), and on box meshes of affine cells of order ngl 4..12 (2-D) / 4..8 (3-D) only with ``-pynama_mat_free_ho``; from there
the same rules apply.  ``-pynama_mat_free_ho_general`` (opt-in, one rank) gives ``Mat.K`` of any quadrilateral / hexahedral mesh of
those orders a shell -- bent cells, imported (Gmsh) meshes, any numbering and vertex valence: the Jacobian is formed at every
quadrature point from the cell's corners.  With both options the affine shell is taken where it applies (it is the faster one) and
the general one elsewhere.  ``-pynama_mat_free_ngl3_general`` (opt-in, one rank) does the same at the reference's own order: a
second-order lattice with a cell that is not affine, or an imported quadrilateral / hexahedral mesh lifted to ngl 3, gets a shell
that interpolates to the points of both Gauss rules and forms the Jacobian there; with ``-pynama_mat_free_ngl3`` as well, the
affine shell is tried first.  ``-pc_type mg`` stays refused on meshes that are no lattice, with or without a shell, and does not
multiply with the general ngl 3 shell (the V-cycle keeps the assembled product).

The reference's hard-wired default is ``preonly`` + ``lu`` (:13-16).  Systems of up to ``-pynama_direct_max_rows`` rows
(default 8192 = the library's limit; one rank) ARE solved directly: ``pyn_solve_direct`` factors the matrix densely with partial pivoting once
per matrix version and every call is two triangular solves -- the sizes at which the reference's own tests use the default
(src/tests/test_solver.py: 882 .. 1,029 unknowns).  There is no sparse direct solver on the device path: above that size
(or on several ranks) the combination is served by a Krylov solve driven to round-off --
Jacobi-PCG (rtol 1e-14 on the recurrence residual, the true residual checked at exit) when a
symmetry probe of the operator passes (``v'Au == u'Av`` on two random vectors, once per operator),
GMRES(30)+Jacobi otherwise or when PCG breaks down (an indefinite operator, e.g. ``K + Kfs`` with its
-1 diagonal entries, base_problem.py:229).  A direct solver either solves or raises: so does this
path -- a negative converged reason or a true residual above 1e-8 raises instead of returning
garbage.  The substitution is logged; it satisfies the reference's own analytic assertions
(src/tests/test_solver.py:20-62).

``-pynama_direct_band`` (opt-in, off by default; PETSc's analogue is picking a factorisation package with
``-pc_factor_mat_solver_type``): above the dense limit, ``preonly`` + ``lu``/``cholesky`` on one rank factors the matrix in band
storage instead (``pyn_solve_direct_band``: LU with partial pivoting, gbtrf semantics, the existing numbering, factors cached per
matrix version) -- a real direct solve for structured meshes, whose band grows with the mesh face, and for the indefinite
``K + Kfs`` as well.  It is taken unless ``-pynama_mat_free`` was asked for explicitly (a matrix-free tag on ``Mat.K`` does not stop
it: the factors replace the shell) and while the factors fit ``-pynama_direct_band_max_gb`` (default 16 GB).  When the band does not
fit (the cap, the free device memory: e.g. imported meshes, whose numbering is not banded) the reason is logged and the Krylov
substitute above runs; a zero pivot raises.

``-ksp_type cg -pc_type mg`` (PETSc's PCMG): CG preconditioned by one geometric multigrid V-cycle per iteration
(``pyn_mg_setup`` / ``PYN_PC_MG``: Galerkin coarse operators on the structured lattice, Chebyshev-Jacobi smoothing, dense LU on the
coarsest level; one rank, lattice meshes).  Options: ``-pc_mg_levels`` (most levels, the matrix included), ``-mg_levels_ksp_max_it``
(Chebyshev degree, default 2), ``-pynama_mg_coarse_max_rows`` (coarsening stops at this many rows, default 4096).  The hierarchy is
cached in the matrix until its values change.  ``gmres`` or ``preonly`` with ``mg`` is refused in ``setUp``.  With a matrix-free tag
CG multiplies with the shell at level 0 as with Jacobi.  Box meshes of order ngl >= 4 are lattice meshes here too (their level 1 is
the Q1 lattice of the same cells), with or without ``-pynama_mat_free_ho``.
"""
import logging

import numpy as np

from pynama_amd import _lib
from pynama_amd.common.options import Options

_NORMS = {"preconditioned": _lib.NORM_PRECONDITIONED, "unpreconditioned": _lib.NORM_UNPRECONDITIONED,
          "natural": _lib.NORM_NATURAL}


class KspSolver(object):
    def __init__(self):
        self.logger = None
        self.mat = None
        self.ksp_type, self.pc_type = 'preonly', 'lu'
        self.rtol, self.atol, self.divtol, self.max_it = 1e-5, 1e-50, 1e5, 10000     # PETSc defaults
        self.restart = 30
        self.gmres_orthog = 1            # KSPGMRES default: classical Gram-Schmidt, refine_never
        self.norm_type = "preconditioned"
        self.mat_free = None             # None: automatic (the shell when the matrix carries one); True / False: -pynama_mat_free
        self.direct_max_rows = 8192      # preonly/lu: dense LU up to this many rows (the library's limit), the Krylov substitute above
        self.direct_band = False         # -pynama_direct_band: preonly/lu above that limit as a banded LU (one rank)
        self.direct_band_max_gb = 16.0   # -pynama_direct_band_max_gb: cap on the band factors' storage (1e9 bytes)
        self.mg_levels = 0               # -pc_mg_levels (0: the library's default)
        self.mg_degree = 0               # -mg_levels_ksp_max_it: Chebyshev degree (0: default 2)
        self.mg_coarse_max_rows = 0      # -pynama_mg_coarse_max_rows (0: default 4096)
        self.info = None
        self._symmetric = None

    # -- PETSc-style setters the reference (or its users) may call
    def setType(self, t):
        self.ksp_type = t

    def getType(self):
        return self.ksp_type

    def setTolerances(self, rtol=None, atol=None, divtol=None, max_it=None):
        if rtol is not None:
            self.rtol = rtol
        if atol is not None:
            self.atol = atol
        if divtol is not None:
            self.divtol = divtol
        if max_it is not None:
            self.max_it = max_it

    def setFromOptions(self):
        o = Options()
        self.ksp_type = o.getString('ksp_type', self.ksp_type)
        self.pc_type = o.getString('pc_type', self.pc_type)
        self.rtol = o.getReal('ksp_rtol', self.rtol)
        self.atol = o.getReal('ksp_atol', self.atol)
        self.divtol = o.getReal('ksp_divtol', self.divtol)
        self.max_it = o.getInt('ksp_max_it', self.max_it)
        self.restart = o.getInt('ksp_gmres_restart', self.restart)
        self.norm_type = o.getString('ksp_norm_type', self.norm_type)
        self.mat_free = (str(o.getString('pynama_mat_free', '1')).lower() not in ('0', 'false', 'no')
                         if o.hasName('pynama_mat_free') else None)
        self.direct_max_rows = o.getInt('pynama_direct_max_rows', self.direct_max_rows)
        if o.hasName('pynama_direct_band'):
            self.direct_band = str(o.getString('pynama_direct_band', '1')).lower() not in ('0', 'false', 'no')
        self.direct_band_max_gb = o.getReal('pynama_direct_band_max_gb', self.direct_band_max_gb)
        self.mg_levels = o.getInt('pc_mg_levels', self.mg_levels)
        self.mg_degree = o.getInt('mg_levels_ksp_max_it', self.mg_degree)
        self.mg_coarse_max_rows = o.getInt('pynama_mg_coarse_max_rows', self.mg_coarse_max_rows)
        if o.hasName('ksp_gmres_modifiedgramschmidt'):
            self.gmres_orthog = 2
        else:
            ref = o.getString('ksp_gmres_cgs_refinement_type', None)
            if ref is not None:
                if ref not in ('refine_never', 'refine_ifneeded', 'refine_always'):
                    raise ValueError(f"unknown -ksp_gmres_cgs_refinement_type {ref}")
                self.gmres_orthog = 1 if ref == 'refine_never' else 0

    def setOperators(self, mat):
        self.mat = mat
        self._symmetric = None           # not probed yet

    def _probe_symmetry(self, A):
        """|v'Au - u'Av| relative to its terms, on two seeded random vectors (two products, once per operator)"""
        from pynama_amd.vectors import Vec
        ctx = A.ctx
        rng = np.random.default_rng(20240229)
        u, v, Au, Av = (Vec(ctx, A.bc) for _ in range(4))
        n = ctx.n_owned * A.bc
        u.setArray(rng.standard_normal(n))
        v.setArray(rng.standard_normal(n))
        ctx.spmv(A.id, u.id, Au.id)
        ctx.spmv(A.id, v.id, Av.id)
        a, b = v.dot(Au), u.dot(Av)
        return abs(a - b) <= 1e-10 * (abs(a) + abs(b) + 1e-300)

    def setUp(self):
        if self.pc_type == 'mg' and self.ksp_type != 'cg':
            raise ValueError(f"-pc_type mg runs with -ksp_type cg only, not {self.ksp_type}")
        if self.ksp_type == 'preonly' and self.pc_type not in ('lu', 'cholesky'):
            raise ValueError("-ksp_type preonly needs a direct -pc_type")
        if self.ksp_type not in ('cg', 'gmres', 'preonly'):
            raise ValueError(f"unsupported -ksp_type {self.ksp_type}")
        if self.ksp_type != 'preonly' and self.pc_type not in ('jacobi', 'none', 'mg'):
            raise ValueError(f"unsupported -pc_type {self.pc_type} (jacobi | none | mg)")

    def createSolver(self, mat, comm):
        self.logger = logging.getLogger("KSP Solver")
        self.logger.debug("setupKSP")
        self.comm = comm
        self.ksp_type, self.pc_type = 'preonly', 'lu'        # ksp_solver.py:13-16
        self.setFromOptions()                                  # :17
        self.setOperators(mat)                                 # :18
        self.setUp()                                           # :19

    def solve(self, b, x):
        A = self.mat
        mf = _lib.MATFREE_OFF
        tag = getattr(A, 'matfree', None)              # set by the assembly that built the matrix (Mat.assembleKLE)
        if self.mat_free:
            if tag is None:
                raise ValueError("-pynama_mat_free: this operator has no matrix-free form (structured Q1 hex meshes; "
                                 "second-order structured meshes of affine cells with -pynama_mat_free_ngl3; box meshes "
                                 "of affine cells of order ngl 4..12 in 2-D / 4..8 in 3-D with -pynama_mat_free_ho; any "
                                 "quadrilateral / hexahedral mesh of those orders on one rank with -pynama_mat_free_ho_general, "
                                 "of order ngl 3 with -pynama_mat_free_ngl3_general)")
            mf = tag
        elif self.mat_free is None and tag is not None and self.ksp_type in ('cg', 'preonly'):
            try:                                       # automatic: the shell, unless the library finds it differs from A
                return self._solve(A, b, x, tag)
            except _lib.PynamaHipError as e:
                if "matrix-free operator differs" not in str(e):
                    raise
                self.logger and self.logger.warning(f"{e}; solving with the assembled matrix")
                A.matfree = None
        return self._solve(A, b, x, mf)

    def _solve(self, A, b, x, mf):
        ctx = A.ctx
        self.shell_used = bool(mf)                     # which product the Krylov loop multiplies with
        n_rows = ctx.n_owned * A.br
        if (self.ksp_type == 'preonly' and not self.mat_free and A.br == A.bc and ctx.nranks == 1 and ctx.n_ghost == 0
                and n_rows <= min(self.direct_max_rows, ctx.direct_max_rows())):
            info = ctx.solve_direct(A.id, b.id, x.id)          # raises on a zero pivot
            if info.reason < 0 or not (info.true_resid <= 1e-8):
                raise RuntimeError(f"preonly/lu: dense LU of {n_rows} rows left a true residual of {info.true_resid:.3e} "
                                   "(the matrix is singular to working precision)")
        elif self.ksp_type == 'preonly' and (info := self._solve_band(A, b, x, n_rows)) is not None:
            self.shell_used = False
        elif self.ksp_type == 'preonly':
            if getattr(self, "_symmetric", None) is None:
                self._symmetric = A.br == A.bc and self._probe_symmetry(A)
            info = None
            if self._symmetric:
                self.logger and self.logger.info("preonly/lu requested: device path uses Jacobi-PCG to round-off")
                info = ctx.solve(A.id, b.id, x.id, method=_lib.KSP_CG, pc=_lib.PC_JACOBI, rtol=1e-14, atol=1e-300,
                                 dtol=1e8, maxit=200000, norm_type=_lib.NORM_UNPRECONDITIONED, matfree=mf)
            if info is None or info.reason < 0:
                why = "operator not symmetric" if not self._symmetric else f"PCG ended with reason {info.reason}"
                self.logger and self.logger.warning(f"preonly/lu requested: {why}; GMRES(30)+Jacobi to round-off instead")
                info = ctx.solve(A.id, b.id, x.id, method=_lib.KSP_GMRES, pc=_lib.PC_JACOBI, rtol=1e-13, atol=1e-300,
                                 dtol=1e8, maxit=200000, restart=30, gmres_orthog=0, norm_type=_lib.NORM_UNPRECONDITIONED)
            if info.reason < 0 or not (info.true_resid <= 1e-8):
                raise RuntimeError(f"preonly/lu substitute failed: converged reason {info.reason}, true residual "
                                   f"{info.true_resid:.3e} after {info.iters} iterations (a direct solver would have solved "
                                   "this system or raised)")
        else:
            if self.pc_type == 'mg':        # no-op unless the options or the values changed since the last build
                ctx.mg_setup(A.id, max_levels=self.mg_levels, smooth_degree=self.mg_degree,
                             coarse_max_rows=self.mg_coarse_max_rows)
            info = ctx.solve(A.id, b.id, x.id,
                             method=_lib.KSP_CG if self.ksp_type == 'cg' else _lib.KSP_GMRES,
                             pc={'jacobi': _lib.PC_JACOBI, 'mg': _lib.PC_MG}.get(self.pc_type, _lib.PC_NONE),
                             rtol=self.rtol, atol=self.atol, dtol=self.divtol, maxit=self.max_it,
                             restart=self.restart, norm_type=_NORMS[self.norm_type], gmres_orthog=self.gmres_orthog,
                             matfree=mf)
            if info.reason < 0 and self.logger:      # PETSc does not raise either (unless -ksp_error_if_not_converged)
                self.logger.error(f"KSP did not converge: reason {info.reason} after {info.iters} iterations, residual {info.rnorm:.3e}")
        self.info = info
        return info

    def _solve_band(self, A, b, x, n_rows):
        """-pynama_direct_band: the banded LU, or None (with the reason logged) when it does not apply or does not fit"""
        ctx = A.ctx
        if not self.direct_band or self.mat_free:
            return None
        why = None
        if ctx.nranks != 1 or ctx.n_ghost != 0:
            why = f"{ctx.nranks} ranks (the banded LU runs on one)"
        elif A.br != A.bc:
            why = f"a {A.br} x {A.bc} block matrix is not square"
        else:
            cap = int(self.direct_band_max_gb * 1e9)
            kl, ku, nbytes = ctx.direct_band_info(A.id)
            if nbytes > cap:
                why = (f"its factors (kl {kl}, ku {ku}, {n_rows} rows) take {nbytes / 1e9:.3g} GB, above "
                       f"-pynama_direct_band_max_gb {self.direct_band_max_gb:g}")
            else:
                try:
                    info = ctx.solve_direct_band(A.id, b.id, x.id, max_bytes=cap)
                except _lib.PynamaHipError as e:
                    if "zero pivot" in str(e):
                        raise
                    why = str(e)
        if why is not None:
            self.logger and self.logger.warning(f"preonly/lu: no banded LU: {why}; Krylov substitute instead")
            return None
        if info.reason < 0 or not (info.true_resid <= 1e-8):
            raise RuntimeError(f"preonly/lu: banded LU of {n_rows} rows left a true residual of {info.true_resid:.3e} "
                               "(the matrix is singular to working precision)")
        self.logger and self.logger.info(f"preonly/lu: banded LU of {n_rows} rows (kl {kl}, ku {ku})")
        return info

    __call__ = solve

    def getIterationNumber(self):
        return self.info.iters if self.info else 0

    def getResidualNorm(self):
        return self.info.rnorm if self.info else 0.0

    def getConvergedReason(self):
        return self.info.reason if self.info else 0

    def destroy(self):
        self.mat = None
