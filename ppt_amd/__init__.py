"""ppt_amd: the MI355X-native hot path of auniquesun/PPT."""
import os

# The step runs on two HIP streams (point tower | prompt side).  The runtime deals streams round-robin onto 4 hardware
# queues by default; once RCCL has created its own streams, the text stream can land on the queue of the caller's
# stream, and the two then execute serially (measured: 4.8 -> 6.2 ms per C2 step after init_process_group alone).
# Eight queues keep them apart.  Must be set before the HIP runtime initialises, i.e. import ppt_amd (or bench.py)
# before the first torch.cuda call; an explicit GPU_MAX_HW_QUEUES in the environment wins.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")


# A forked child (the DataLoader's workers: ppt_amd/data/fps_service.py) inherits the parent's whole Python heap, including
# garbage cycles that still hold HIP objects -- graphs, events, streams of models that are gone (the hazard graphs.GraphedCall
# guards its captures against).  Should the child's cyclic collector run before the parent's has, it finalises them, and a HIP
# call in a forked process faults ("Fatal Python error: Segmentation fault ... Garbage-collecting" in the worker's bootstrap,
# whenever an allocation count happened to put a collection there).  The child therefore moves everything it inherited into the
# collector's permanent generation: its own new objects are collected as usual, the parent's are never finalised by it.
def _freeze_inherited_heap():
    import gc
    gc.freeze()


if hasattr(os, "register_at_fork"):
    os.register_at_fork(after_in_child=_freeze_inherited_heap)
