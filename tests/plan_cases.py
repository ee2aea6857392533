"""The symbolic phase on the CPU, for every test that asks the plan something — TEST INFRASTRUCTURE: swf_debug_plan_check
(plan_build + plan_validate, no device) and the batches of clique shapes that tests/test_clique_pack_host.py and
tests/test_imu_record_host.py both validate."""
import ctypes

from rtk_visual_inertial_navigation_amd import build, solver, synth
from rtk_visual_inertial_navigation_amd.flat import FlatWindowC

INFO = ("ls_var", "ls_qpb", "ls_gqpb", "ls_folded", "lat_fuse", "want_aux", "want_Linv", "want_Wk", "asm_programs", "n_pch_split", "max_red", "n_pch")


def plan_check(wins, n_cu=256, ls_variant=0, ls_qpb=0, ls_grad_qpb=0, flags=0, corrupt=(0, 0)):
    """(return code, swf_last_error, info) of swf_debug_plan_check on the windows."""
    build.build()
    lib = ctypes.CDLL(solver.LIB_PATH)
    lib.swf_last_error.restype = ctypes.c_char_p
    cs = [w.c_struct() for w in wins]
    arr = (ctypes.POINTER(FlatWindowC) * len(cs))(*[ctypes.pointer(c) for c in cs])
    info = (ctypes.c_int32 * len(INFO))()
    rc = lib.swf_debug_plan_check(arr, ctypes.c_int32(len(cs)), ctypes.c_int32(n_cu), ctypes.c_int32(ls_variant), ctypes.c_int32(ls_qpb),
                                  ctypes.c_int32(ls_grad_qpb), ctypes.c_int32(flags), ctypes.c_int32(corrupt[0]), ctypes.c_int32(corrupt[1]), info)
    return rc, (lib.swf_last_error() or b"").decode(), dict(zip(INFO, info))


def clique_batches():
    mixed = [synth.make_window(3, seed=910), synth.make_window(3, K=6, F=30, S=5, seed=911), synth.make_window(3, K=6, F=30, S=20, seed=912),
             synth.make_window(3, seed=913), synth.make_window(3, K=6, F=30, S=5, seed=914)]
    # S = 24 satellites: clock cliques of 48 rows x 31 columns (the class's row limit; (31 + 1) | 1 = 33, its largest leading dimension);
    # S = 25 would be 50 rows and leaves class 0
    envelope = [synth.make_window(3, K=6, F=30, S=24, seed=920), synth.make_window(3, seed=921), synth.make_window(3, K=6, F=30, S=5, seed=922)]
    beyond = [synth.make_window(3, K=6, F=30, S=25, seed=923), synth.make_window(3, K=6, F=30, S=5, seed=922)]
    one = [synth.make_window(3, seed=924)]
    free = [synth.make_window(2, K=3, F=5, S=0, seed=3), synth.make_window(3, K=4, F=6, S=2, seed=2)]        # no satellites: the dummy and free groups alone
    return dict(mixed=mixed, envelope=envelope, beyond=beyond, one=one, free=free)
