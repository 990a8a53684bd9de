"""Child process of test_pt_canonical_walks.test_wavefront_knobs_in_fresh_processes: the wavefront tracer's tuning
variables (PTGS_WF_TRACE_RUN, PTGS_WF_SHADE_RUN, PTGS_WF_REFILL, PTGS_WF_BATCH) are read once per process, so each
setting renders in a process of its own, with the variables in its environment.

  python wf_knobs_child.py <out.npz>

Renders, with the wavefront tracer, the features scene at 160x120 and 7 spp from frame 3 (the running mean over a
seeded non-zero accumulator) and the Cornell box at 512x512 and 1 spp (262144 slots: four runs of 65536), and writes
the two images and their (extension, shadow, sample) counts."""
import sys

import numpy as np

import scenes_util as U
from pathtracer_gaussiansplatting_amd import make_ubo

FW, FH, FSPP, FFRAME = 160, 120, 7, 3
CW = CH = 512


def features_case():
    """(scene, ubo, the accumulator's initial contents)."""
    sc = U.features()
    init = np.random.default_rng(7).uniform(0.0, 1.0, (FH, FW, 4)).astype(np.float32)
    return sc, make_ubo(U.cornell_pose(FW / FH), sc, FFRAME, ambient=(0.05, 0.05, 0.08, 1.0)), init


def cornell_case():
    sc = U.cornell()
    return sc, make_ubo(U.cornell_pose(), sc, 0)


def main(out):
    import torch
    from pathtracer_gaussiansplatting_amd import Renderer
    r = Renderer(0, wavefront=True)
    res = {}
    for name, (sc, ubo, init), (w, h, spp) in (("features", features_case(), (FW, FH, FSPP)),
                                               ("cornell", cornell_case() + (None,), (CW, CH, 1))):
        r.upload_scene(sc)
        acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        if init is not None:
            acc.copy_(torch.from_numpy(init))
        r.stats_reset()
        r.trace_camera(ubo, w, h, acc, spp=spp)
        torch.cuda.synchronize()
        st = r.stats()
        res[name] = acc.cpu().numpy()
        res[name + "_counts"] = np.array([st.extension_rays, st.shadow_rays, st.samples], np.int64)
    r.close()
    np.savez(out, **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
