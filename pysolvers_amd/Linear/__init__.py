"""Drop-in for PySolvers.Linear's PCG/GMRES path (Linear/__init__.py:1-12 names)."""
from .AMGPreconditioner import AMG, AMGPreconditioner
from .BiCGStabSolver import BiCGStab, BiCGStabSolver
from .ClassicSmoothers import (ChebyshevSmoother, GaussSeidelSmoother, JacobiSmoother,
                               MulticolorGaussSeidelSmoother)
from .DeviceMatrix import DeviceCSR, DeviceVector, matmat, spmv
from .DirectSolver import DefaultDirect, DefaultDirectSolver
from .Distributed import Communicator, fd_laplacian_2d_sharded, halo_cols, shard_csr
from .GMRESSolver import GMRES, GMRESSolver
from .IDRsSolver import IDRs, IDRsSolver
from .ILUTPreconditioner import (ILUTPreconditioner, LeftILUT, LeftILUTPreconditioner, RightILUT,
                                 RightILUTPreconditioner)
from .ILU0Preconditioner import (ILU0Preconditioner, LeftILU0, LeftILU0Preconditioner, RightILU0,
                                 RightILU0Preconditioner)
from .ILUKPreconditioner import (ILUKPreconditioner, LeftILUK, LeftILUKPreconditioner, RightILUK,
                                 RightILUKPreconditioner)
from .ICPreconditioner import ICRightPreconditioner, RightIC
from .IterativeLinearSolver import IterativeLinearSolver, IterativeLinearSolverType, mvmult
from .LinearSolver import LinearSolver, LinearSolverType
from .MINRESSolver import MINRES, MINRESSolver
from .PCGSolver import PCG, PCGSolver
from .MLHierarchy import MLHierarchy, makeRestrictionOp
from .Preconditioner import (ChebyshevPreconditioner, DeviceOperator, FSAIPreconditioner, GenericPreconditioner,
                             IdentityPreconditioner, JacobiPreconditioner, LeftPreconditioner, MulticolorGSPreconditioner,
                             Preconditioner, RightPreconditioner)
from .PreconditionerType import (Chebyshev, ChebyshevPreconditionerType, FSAI, FSAIPreconditionerType,
                                 IdentityPreconditionerType, Jacobi,
                                 JacobiPreconditionerType, MulticolorGS, MulticolorGSPreconditionerType,
                                 PreconditionerType)
from .SmoothedAggregation import SA_coarsen, SmoothedAggregationMLHierarchy
from .TriangularSolve import TriangularSolveChain
from .VCycleSolver import AMGVCycle, AMGVCycleSolver
