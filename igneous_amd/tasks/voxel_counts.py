"""CountVoxelsTask — drop-in for igneous.tasks.CountVoxelsTask
(igneous/tasks/image/image.py:849-884): download one unpadded task box,
count the voxels of every label, write
"{key}/stats/voxel_counts/{bbox}.json" as {str(segid): count}, 0 included.
accumulate_voxel_counts (task_creation/voxel_counts.py) sums the files into
the voxel_counts.im sidecar MeshTask's dust_global reads.

The count crosses to the GPU where the reference calls fastremap.unique
(image.py:876): the mesher's count_voxels, the HIP engine's mg_count_voxels.
There is no CPU fallback; a mesher without a counter raises.
"""
from __future__ import annotations

from ..lib import Bbox, Vec
from ..queue import RegisteredTask
from ..storage import CloudFiles
from ..volume import PrecomputedVolume
from .mesh import _get_mesher


def voxel_counts_dir(key: str) -> str:
    return f"{key}/stats/voxel_counts"


def voxel_counts_sidecar(key: str) -> str:
    return f"{key}/stats/voxel_counts.im"


class CountVoxelsTask(RegisteredTask):
    def __init__(self, cloudpath, shape, offset, mip=0, fill_missing=False,
                 agglomerate=False, timestamp=None):
        super().__init__(cloudpath, shape, offset, mip, fill_missing,
                         agglomerate, timestamp)
        if agglomerate or timestamp is not None:
            raise NotImplementedError(
                "agglomerate / timestamp need a graphene server; only "
                "precomputed volumes are counted")
        self.cloudpath = cloudpath
        self.shape = Vec(*shape)
        self.offset = Vec(*offset)
        self.mip = int(mip)
        self.fill_missing = bool(fill_missing)

    def execute(self):
        counter = getattr(_get_mesher(), 'count_voxels', None)
        if counter is None:
            raise NotImplementedError(
                "CountVoxelsTask needs a mesher that counts voxels "
                "(count_voxels): the HIP engine does, the injected mesher "
                "does not")
        vol = PrecomputedVolume(self.cloudpath, self.mip, bounded=False,
                                fill_missing=self.fill_missing)
        # no padding: neighbouring tasks never count a voxel twice
        bbox = Bbox.clamp(Bbox(self.offset, self.offset + self.shape),
                          vol.bounds)
        labels = vol.download(bbox)[..., 0]
        values, counts = counter(labels)
        CloudFiles(self.cloudpath).put_json(
            f"{voxel_counts_dir(vol.key)}/{bbox.to_filename()}.json",
            {str(int(segid)): int(ct) for segid, ct in zip(values, counts)})
