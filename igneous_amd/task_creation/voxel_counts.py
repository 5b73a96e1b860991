"""create_voxel_counting_tasks / accumulate_voxel_counts — drop-ins for the
reference generators at igneous/task_creation/image.py:1928-2030: 512^3
CountVoxelsTasks over a volume, then the sum of their JSON files into the
IntMap sidecar "{key}/stats/voxel_counts.im" that MeshTask's dust_global
reads.
"""
from __future__ import annotations

from collections import defaultdict
from time import strftime
from typing import Optional

import numpy as np

from ..formats.intmap import IntMap
from ..lib import Bbox, Vec
from ..storage import CloudFiles
from ..tasks.voxel_counts import (CountVoxelsTask, voxel_counts_dir,
                                  voxel_counts_sidecar)
from ..volume import PrecomputedVolume
from .common import FinelyDividedTaskIterator, operator_contact

__all__ = ["create_voxel_counting_tasks", "accumulate_voxel_counts"]

COUNT_TASK_SHAPE = (512, 512, 512)


def _bounded(shape, offset, bounds: Bbox) -> Vec:
    """The task shape cut at the volume's upper edge (image.py:1945)."""
    return Vec(*np.minimum(shape, bounds.maxpt - offset))


def create_voxel_counting_tasks(cloudpath: str, mip: int,
                                fill_missing: bool = False,
                                shape=COUNT_TASK_SHAPE):
    """Count voxels in 512^3 tasks; each writes
    $KEY/stats/voxel_counts/$BBOX.json."""
    vol = PrecomputedVolume(cloudpath, mip)
    shape = Vec(*shape)
    bounds = vol.bounds.clone()

    class CountVoxelsTaskIterator(FinelyDividedTaskIterator):
        def task(self, shape, offset):
            return CountVoxelsTask(
                cloudpath=cloudpath,
                shape=_bounded(shape, offset, bounds),
                offset=offset.clone(),
                mip=mip,
                fill_missing=fill_missing,
            )

        def on_finish(self):
            vol.provenance.processing.append({
                'method': {
                    'task': 'CountVoxelsTask',
                    'cloudpath': cloudpath,
                    'mip': mip,
                    'shape': shape.tolist(),
                    'fill_missing': fill_missing,
                    'agglomerate': False,
                    'timestamp': None,
                },
                'by': operator_contact(),
                'date': strftime('%Y-%m-%d %H:%M %Z'),
            })
            vol.commit_provenance()

    return CountVoxelsTaskIterator(bounds, shape)


def accumulate_voxel_counts(cloudpath: str, mip: int, progress: bool = True,
                            compress: Optional[str] = None,
                            additional_output: Optional[str] = None,
                            shape=COUNT_TASK_SHAPE):
    """Sum every task's counts into $KEY/stats/voxel_counts.im (an IntMap).
    A task file that is not there raises FileNotFoundError naming it."""
    vol = PrecomputedVolume(cloudpath, mip)
    bounds = vol.bounds.clone()

    class BboxIterator(FinelyDividedTaskIterator):
        def task(self, shape, offset):
            return Bbox(offset, offset + _bounded(shape, offset, bounds))

    cf = CloudFiles(cloudpath)
    final_counts = defaultdict(int)
    for bbx in BboxIterator(bounds, Vec(*shape)):
        name = f"{voxel_counts_dir(vol.key)}/{bbx.to_filename()}.json"
        counts = cf.get_json(name)
        if counts is None:
            raise FileNotFoundError(
                f"voxel counts of {bbx.to_filename()} are missing: "
                f"{cloudpath.rstrip('/')}/{name} (run the CountVoxelsTasks "
                f"first)")
        for segid, ct in counts.items():
            final_counts[int(segid)] += int(ct)

    binary = IntMap(final_counts).tobytes()
    if additional_output:
        with open(additional_output, "wb") as f:
            f.write(binary)
    cf.put(voxel_counts_sidecar(vol.key), binary,
           content_type="application/x-intmap", compress=compress)
