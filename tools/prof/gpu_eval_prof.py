"""Phase stamps of the projection segment of k_eval_ps (block 0, thread 0) — needs a library built with -DSWF_PROFILE_EVAL:
   SWF_EXTRA_FLAGS=-DSWF_PROFILE_EVAL python -m rtk_visual_inertial_navigation_amd.build; python tools/prof/gpu_eval_prof.py [windows]"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
from rtk_visual_inertial_navigation_amd import synth, solver
from rtk_visual_inertial_navigation_amd.flat import default_options
B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
ws = bench.make_windows(4, [synth.BASE_SEED + 4 + i for i in range(B)])
bs = solver.BatchSolver(ws)
for _ in range(3):
    bs.reset_state(); bs.solve(default_options(step_mode=1), download=False)
out = (C.c_ulonglong * 16)()
solver.lib().swf_debug_eval_stamps(out)
s = list(out)
print("windows", B, "| block record", s[0], "| indices + window constants", s[1], "| state values", s[2], "| proj_core + stores", s[3],
      "| block cost", s[4], "| frame sums", s[5], "| total", sum(s[:6]), "(s_memtime ticks; frame-sum block 0)")
