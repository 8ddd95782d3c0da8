"""Alternating least squares with approximate recommend / similar_items (the reference's implicit/approximate_als.py).

One wrapper exists: the native IVF-Flat index of implicit_amd.ann.  annoy and nmslib have no counterpart here."""
import implicit_amd.als
import implicit_amd.gpu
from implicit_amd.ann import IVFModel


def IVFAlternatingLeastSquares(*args, approximate_similar_items=True, approximate_recommend=True, nlist=400, nprobe=20,
                               use_gpu=None, **kwargs):
    """An implicit_amd.als.AlternatingLeastSquares model (`args` / `kwargs`) wrapped in an IVFModel of `nlist` lists that scans
    `nprobe` of them per query.  Also bound as FaissAlternatingLeastSquares, whose signature it has: the index is this
    package's native IVF-Flat index (implicit_amd.gpu.IVFIndex, the structure of faiss.GpuIndexIVFFlat), NOT faiss, which
    is neither needed nor used.  use_gpu=False raises as implicit_amd.als does: only the MI355X path exists.
    `iterations` and `random_state` keep their ALS meaning; the index build uses its defaults (10 k-means rounds) and the
    same random_state."""
    if use_gpu is None:
        use_gpu = implicit_amd.gpu.HAS_CUDA
    als_model = implicit_amd.als.AlternatingLeastSquares(*args, use_gpu=use_gpu, **kwargs)
    random_state = kwargs.get("random_state")
    return IVFModel(als_model, approximate_similar_items=approximate_similar_items, approximate_recommend=approximate_recommend,
                    nlist=nlist, nprobe=nprobe, random_state=random_state if isinstance(random_state, (int, type(None))) else None)


FaissAlternatingLeastSquares = IVFAlternatingLeastSquares
