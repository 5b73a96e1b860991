"""MeshTask — drop-in for igneous.tasks.MeshTask, MI355X-native compute.

Mirrors the reference class (igneous/tasks/mesh/mesh.py, "mesh.py" below):
  - ctor signature (shape, offset, layer_path, **kwargs) and the full
    options dict of mesh.py:98-129 (kwargs surface preserved verbatim);
  - execute() flow of mesh.py:140-265: clamp bounds, pad by
    low_padding/high_padding (1vx overlap for seam-free stitching,
    mesh.py:155-160), download F-order chunk, zero-border closed dataset
    edges (mesh.py:267-303), dust/remap/object-id masking
    (mesh.py:193-204), mesh every label, shift vertices into global nm
    (mesh.py:434-435), precomputed-encode (mesh.py:448), upload fragments
    named "{mesh_dir}/{segid}:{lod}:{bbox}" (mesh.py:409) plus optional
    manifests (mesh.py:419-430) and spatial index (mesh.py:452-464).

The compute crosses to the GPU exactly where the reference crosses into
zmesh C++ (mesh.py:245 and mesh.py:374-381). execute() fetches the mesher
once, reads what it advertises (set_mesher states the protocol) and calls it
once: the HIP engine's mg_mesh_chunk gives all labels' welded (and optionally
simplified) meshes. When advertised, the same call carries, as device passes:
  - handles_dust / handles_label_map: dust_threshold and the label selection
    (remap_table / object_ids / exclude_object_ids, folded by
    remap.fold_label_ops) — _select_labels decides host or device;
  - handles_dust_global: dust_threshold with dust_global (mesh.py:324-355):
    the chunk's labels are counted on the device (mg_count_voxels), looked
    up in the voxel_counts.im sidecar that accumulate_voxel_counts wrote, and
    the labels below the threshold folded into the label map;
  - handles_fill_holes: fill_holes levels 1-2 (mesh.py:211-243) after dust
    and the selection; the filled and the hole volume's meshes come back
    and are concatenated per segment id;
  - encode_chunk, for the task's encoding: the per-label loop after the
    mesher (shift, box, encode — encode_fragment below); the engine returns
    finished bytes and boxes (mg_mesh_chunk_encoded), the task uploads them.
There is no CPU fallback; a missing engine raises.

Deliberate deviations (documented in DESIGN.md):
  - fastremap.renumber+invert (mesh.py:206-207) is omitted: the engine
    hashes raw labels, so the composition is the identity.
  - dry_run returns (meshes, bounding_boxes) computed; the reference's
    dry_run references bounding_boxes before assignment (mesh.py:249-252,
    a latent NameError).
  - fill_holes 1-2 follow this repository's own written contract
    (fastmorph's source is not available to pin against);
    fill_holes>=3 (multilabel dilation, merge threshold) raises
    NotImplementedError. Sharded output uses the in-repo MapBuffer
    restatement, dust_global the in-repo IntMap restatement and draco
    encoding the in-repo Draco restatement (formats/, byte-level external
    parity unpinned offline — DESIGN.md §7).
"""
from __future__ import annotations

import numpy as np

from ..lib import Bbox, Vec
from ..meshes import Mesh
from ..queue import RegisteredTask
from ..storage import CloudFiles
from ..volume import PrecomputedVolume
from .. import remap as fastremap_np

# Product mesher: the HIP engine. Tests may swap this seam to run host-logic
# tests without a GPU (the swapped-in callable is then the *checker's*
# oracle, never shipped); the default import path is GPU-only.
_mesher_fn = None
# {sidecar path: IntMap} of the global voxel counts (dust_global)
_voxel_counts_cache: dict = {}


def set_mesher(fn) -> None:
    """Test seam. Pass None to restore the HIP product engine.

    The protocol: execute() calls fn(data, resolution=, reduction_factor=,
    max_error=, voxel_centered=, copy=) ONCE and takes its {label: (verts,
    faces)}. fn accepts `copy` (False: the result may alias storage that
    lives until fn's next call) and every keyword it advertises by
    attribute: handles_dust -> dust_threshold=, handles_label_map ->
    label_map=(keys, vals, miss), handles_dust_global ->
    dust_global=(threshold, lookup) with lookup(labels_u64) -> global voxel
    counts_u64 (fn erases the chunk's labels below the threshold before the
    label map; never together with dust_threshold=), handles_fill_holes ->
    fill_holes= (the result is then the pair (filled, holes)), count_voxels
    -> a callable (3-D labels) -> (values, counts) as np.unique gives them
    (CountVoxelsTask, and dust_global where the label map stays on the
    host), encode_chunk -> a second
    callable taking the same keywords plus shift= / encoding= / draco= and
    returning an engine.EncodedChunk, for the encodings its `formats` lists
    (all, if it has none). What fn raises, TypeError included, reaches
    execute()'s caller: there is no second call."""
    global _mesher_fn
    _mesher_fn = fn


def _get_mesher():
    if _mesher_fn is not None:
        return _mesher_fn
    from .. import engine
    return engine.mesh_chunk


class _Capabilities:
    """What a mesher advertises (set_mesher's protocol), read here only."""

    def __init__(self, mesher):
        self.dust = getattr(mesher, 'handles_dust', False)
        self.label_map = getattr(mesher, 'handles_label_map', False)
        self.fill_holes = getattr(mesher, 'handles_fill_holes', False)
        self.dust_global = getattr(mesher, 'handles_dust_global', False)
        self.count_voxels = getattr(mesher, 'count_voxels', None)
        self.encode_chunk = getattr(mesher, 'encode_chunk', None)
        self.formats = getattr(self.encode_chunk, 'formats', None)


def encode_fragment(mesh: Mesh, shift, encoding: str, draco_settings=None):
    """One label's step of the host loop: shift the mesh's vertices IN
    PLACE into global nm, take their box, encode. -> (bytes, box), box the
    flat [minx,miny,minz,maxx,maxy,maxz] of Bbox.to_list() (mesh.py:257).

    This is the contract of the engine's device encode stage
    (mg_mesh_chunk_encoded gives the same bytes and an == box for every
    label); the fallback loop and the tests' checker both call it."""
    mesh.vertices[:] += shift
    mesh_bounds = (np.amin(mesh.vertices, axis=0).tolist()
                   + np.amax(mesh.vertices, axis=0).tolist())
    if encoding == 'draco':
        # mesh.py:442-446 via our draco restatement (formats/draco.py)
        from ..formats import draco as draco_fmt
        binary = draco_fmt.encode(
            mesh.vertices, mesh.faces, **draco_settings)
        return binary, mesh_bounds
    return mesh.to_precomputed(), mesh_bounds


class MeshTask(RegisteredTask):
    def __init__(self, shape, offset, layer_path, **kwargs):
        """Convert all labels in the bounding box into meshes via marching
        cubes and quadric edge collapse on the MI355X HIP engine.

        Required:
          shape: (sx,sy,sz) size of task
          offset: (x,y,z) offset from (0,0,0)
          layer_path: neuroglancer/precomputed dataset path (file://)

        Optional kwargs: identical to the reference MeshTask
        (mesh.py:40-129): lod, mip, simplification_factor,
        max_simplification_error, mesh_dir, remap_table,
        generate_manifests, low_padding, high_padding, parallel_download,
        cache_control, dust_threshold, dust_global, encoding,
        draco_compression_level, draco_create_metadata, progress,
        object_ids, exclude_object_ids, fill_missing, spatial_index,
        sharded, timestamp, agglomerate, stop_layer, compress,
        closed_dataset_edges, fill_holes, dry_run, frag_path.
        """
        super().__init__(shape, offset, layer_path, **kwargs)
        self.shape = Vec(*shape)
        self.offset = Vec(*offset)
        self.layer_path = layer_path
        self.options = {
            'cache_control': kwargs.get('cache_control', None),
            'draco_compression_level': kwargs.get('draco_compression_level', 1),
            'draco_create_metadata': kwargs.get('draco_create_metadata', False),
            'dust_threshold': kwargs.get('dust_threshold', None),
            'dust_global': kwargs.get('dust_global', False),
            'encoding': kwargs.get('encoding', 'precomputed'),
            'fill_missing': kwargs.get('fill_missing', False),
            'generate_manifests': kwargs.get('generate_manifests', False),
            'high_padding': kwargs.get('high_padding', 1),
            'low_padding': kwargs.get('low_padding', 0),
            'lod': kwargs.get('lod', 0),
            'max_simplification_error': kwargs.get('max_simplification_error', 40),
            'simplification_factor': kwargs.get('simplification_factor', 100),
            'mesh_dir': kwargs.get('mesh_dir', None),
            'frag_path': kwargs.get('frag_path', None),
            'mip': kwargs.get('mip', 0),
            'object_ids': kwargs.get('object_ids', None),
            'exclude_object_ids': kwargs.get('exclude_object_ids', []),
            'parallel_download': kwargs.get('parallel_download', 1),
            'progress': kwargs.get('progress', False),
            'remap_table': kwargs.get('remap_table', None),
            'spatial_index': kwargs.get('spatial_index', False),
            'sharded': kwargs.get('sharded', False),
            'timestamp': kwargs.get('timestamp', None),
            'agglomerate': kwargs.get('agglomerate', True),
            'stop_layer': kwargs.get('stop_layer', 2),
            'compress': kwargs.get('compress', 'gzip'),
            'closed_dataset_edges': kwargs.get('closed_dataset_edges', True),
            'fill_holes': kwargs.get('fill_holes', 0),
            'dry_run': kwargs.get('dry_run', False),
        }
        supported_encodings = ['precomputed', 'draco']
        if self.options['encoding'] not in supported_encodings:
            raise ValueError('Encoding {} is not supported. Options: {}'.format(
                self.options['encoding'], ', '.join(supported_encodings)))
        self._encoding_to_compression_dict = {
            'precomputed': self.options['compress'],
            'draco': False,
        }

    # ------------------------------------------------------------------
    def execute(self):
        opts = self.options
        mesher = _get_mesher()
        can = _Capabilities(mesher)
        fill_level = int(opts['fill_holes'] or 0)
        if fill_level >= 3:
            raise NotImplementedError(
                "fill_holes>=3 is not implemented: level 3 needs "
                "fastmorph's multilabel dilation and levels >= 4 its "
                "merge_threshold, whose tie rules cannot be restated "
                "without the fastmorph source (DESIGN.md §7)")
        if fill_level > 0 and not can.fill_holes:
            raise NotImplementedError(
                "fill_holes>0 needs a mesher that fills holes itself "
                "(handles_fill_holes): the HIP engine does, the injected "
                "mesher does not")

        data, left_offset = self._download()
        if data is None:
            return
        data, call_kw = self._select_labels(data, can)
        # the keywords every mesher call carries (set_mesher's protocol)
        call_kw.update(
            resolution=tuple(float(r) for r in self._volume.resolution),
            reduction_factor=int(opts['simplification_factor'] or 0),
            max_error=float(opts['max_simplification_error']),
            voxel_centered=True)

        # A mesher that advertises encode_chunk returns every label's
        # finished bytes and box from one call (the engine's device encode
        # stage) — no Mesh per label, no host loop. Not with fill_holes
        # (filled and hole meshes are concatenated on the host) nor under
        # dry_run (the caller wants the meshes).
        if (can.encode_chunk is not None and fill_level == 0
                and not opts['dry_run']
                and (can.formats is None or opts['encoding'] in can.formats)):
            encoded = self._encode_on_device(
                can.encode_chunk, data, call_kw, left_offset)
            if encoded is not None:
                del data
                self._upload(*encoded)
                return

        if fill_level:
            # after dust and the label selection, host or device
            # (mesh.py:193-228); the mesher returns (filled, holes)
            call_kw['fill_holes'] = fill_level
        # copy=False: this task consumes (shifts, encodes, uploads) every
        # mesh before its next engine call, so zero-copy views into the
        # engine's staging buffers are safe — EXCEPT under dry_run, where
        # the meshes are handed back to the caller and must own their
        # storage (the reference returns owned arrays).
        raw = mesher(data, copy=bool(opts['dry_run']), **call_kw)
        del data
        meshes, binaries, bounding_boxes = self._host_loop(
            raw, fill_level, left_offset)
        if opts['dry_run']:
            return (meshes, bounding_boxes)
        self._upload(binaries, bounding_boxes)

    def _download(self):
        """Clamp and pad the task's bounds, download, close the dataset's
        edges. -> (data, left_offset); (None, None) for an all-zero chunk,
        whose (empty) spatial index is written here."""
        opts = self.options
        self._volume = PrecomputedVolume(
            self.layer_path, opts['mip'], bounded=False,
            parallel=opts['parallel_download'],
            fill_missing=opts['fill_missing'])
        self._bounds = Bbox.clamp(
            Bbox(self.offset, self.shape + self.offset), self._volume.bounds)

        # 1vx overlap for seam-free stitching between adjacent tasks
        data_bounds = self._bounds.clone()
        data_bounds.minpt -= opts['low_padding']
        data_bounds.maxpt += opts['high_padding']

        self._mesh_dir = self.get_mesh_dir()
        if opts['encoding'] == 'draco':
            from .draco import draco_encoding_settings
            self.draco_encoding_settings = draco_encoding_settings(
                shape=(self.shape + opts['low_padding']
                       + opts['high_padding']),
                offset=self.offset,
                resolution=self._volume.resolution,
                compression_level=opts['draco_compression_level'],
                create_metadata=opts['draco_create_metadata'],
                uses_new_draco_bin_size=False,
            )

        data = self._volume.download(data_bounds)
        if not np.any(data):
            if opts['spatial_index']:
                self._upload_spatial_index(self._bounds, {})
            return None, None
        if opts['closed_dataset_edges']:
            return self._handle_dataset_boundary(data, data_bounds)
        return data, Vec(0, 0, 0)

    def _select_labels(self, data, can):
        """Dust removal and the label selection (remap_table / object_ids /
        exclude_object_ids), each on the device when the mesher can and on
        the host otherwise. -> (3-D data, the dust_threshold / label_map
        keywords that hand the device its share)."""
        opts = self.options
        if opts['remap_table'] is not None:
            opts['remap_table'] = {
                int(k): int(v) for k, v in opts['remap_table'].items()}

        # the selection folded into ONE lookup table, applied by the engine
        # in a device volume pass; meshers that do not advertise it — and
        # folds above the engine's table cap — keep the host
        # mask_except/remap/mask sequence
        label_map = None
        if can.label_map:
            label_map = fastremap_np.fold_label_ops(
                opts['remap_table'], opts['object_ids'],
                opts['exclude_object_ids'], data.dtype)
            if label_map is not None:
                from ..engine import LABEL_MAP_MAX_ENTRIES
                if len(label_map[0]) > LABEL_MAP_MAX_ENTRIES:
                    label_map = None

        call_kw = {}
        if opts['dust_threshold'] and opts['dust_global']:
            # the global threshold: a label is dust by its voxel count over
            # the whole dataset, not over this chunk (mesh.py:324-355)
            if not can.dust_global:
                raise NotImplementedError(
                    "dust_global needs a mesher that takes the global "
                    "voxel counts (handles_dust_global): the HIP engine "
                    "does, the injected mesher does not")
            lookup = self._global_voxel_counts().lookup
            threshold = int(opts['dust_threshold'])
            host_map = (opts['remap_table'] is not None or opts['object_ids']
                        or opts['exclude_object_ids']) and label_map is None
            if can.label_map and not host_map:
                call_kw['dust_global'] = (threshold, lookup)
            else:
                # the label map stays on the host, and dust comes before
                # it: count on the device, mask here
                if can.count_voxels is None:
                    raise NotImplementedError(
                        "dust_global with a host label selection needs the "
                        "mesher's count_voxels")
                values, _ = can.count_voxels(data[..., 0])
                values = np.asarray(values, dtype=np.uint64)
                values = values[values != 0]
                dust = values[lookup(values) < np.uint64(threshold)]
                data = fastremap_np.mask(data, dust.tolist(), in_place=True)
        elif (opts['dust_threshold']
                and (opts['remap_table'] is None or label_map is not None)
                and can.dust):
            # three HIP volume passes instead of a multi-second host
            # unique/mask at 512^3. A HOST remap must force host dust: the
            # reference dusts BEFORE remapping (mesh.py:193-198), so labels
            # merged by the remap pool their voxel counts — device dust
            # would run after the host remap and see the merged labels.
            # With the device label map the engine's order is dust -> map,
            # the reference's order, so both run on the device.
            call_kw['dust_threshold'] = int(opts['dust_threshold'])
        else:
            data = self._remove_dust(data, opts['dust_threshold'])

        if label_map is not None:
            call_kw['label_map'] = label_map
        else:
            data = self._remap(data)
            if opts['object_ids']:
                data = fastremap_np.mask_except(data, opts['object_ids'], in_place=True)
            if opts['exclude_object_ids']:
                data = fastremap_np.mask(data, opts['exclude_object_ids'], in_place=True)
        return data[..., 0], call_kw

    def _encode_on_device(self, encode_chunk, data, call_kw, left_offset):
        """One encode_chunk call -> (binaries, bounding_boxes) by segid.
        None when a label came back without vertices: the host loop decides
        what happens then (np.amin raises on it today)."""
        opts = self.options
        draco = None
        if opts['encoding'] == 'draco':
            draco = dict(self.draco_encoding_settings)
            # arrives as a numpy float (np.ceil)
            draco['quantization_bits'] = int(draco['quantization_bits'])
        encoded = encode_chunk(
            data, shift=self._global_shift(left_offset),
            encoding=opts['encoding'], draco=draco, copy=False, **call_kw)
        if np.any(np.asarray(encoded.nverts) == 0):
            return None
        items = list(encoded.items())
        return ({segid: binary for segid, binary, _ in items},
                {segid: box for segid, _, box in items})

    def _host_loop(self, raw, fill_level, left_offset):
        """The mesher's result -> (meshes, binaries, bounding_boxes) by
        segid: a Mesh per label, shifted, boxed and encoded on the host."""
        hole_raw = {}
        if fill_level:
            raw, hole_raw = raw
        meshes = {
            int(label): Mesh(verts, faces, id=int(label))
            for label, (verts, faces) in raw.items()
        }
        # mesh.py:238-242: a segment's hole mesh is appended to its filled
        # mesh; a segment present only in the hole volume keeps that alone
        for label, (verts, faces) in hole_raw.items():
            segid = int(label)
            hole_mesh = Mesh(verts, faces, id=segid)
            if segid in meshes:
                meshes[segid] = Mesh.concatenate(
                    meshes[segid], hole_mesh, id=segid)
            else:
                meshes[segid] = hole_mesh

        binaries, bounding_boxes = {}, {}
        for segid, mesh in meshes.items():
            binary, mesh_bbx = self._create_mesh_binary(mesh, left_offset)
            binaries[segid] = binary
            bounding_boxes[segid] = mesh_bbx
        return meshes, binaries, bounding_boxes

    def _upload(self, binaries, bounding_boxes):
        opts = self.options
        if opts['sharded']:
            self._upload_batch(binaries, self._bounds)
        else:
            self._upload_individuals(binaries, opts['generate_manifests'])

        if opts['spatial_index']:
            self._upload_spatial_index(self._bounds, bounding_boxes)

    # ------------------------------------------------------------------
    def _handle_dataset_boundary(self, data, bbox):
        """Zero border on sides touching the dataset boundary so meshes
        close there (mesh.py:267-303)."""
        if ((not np.any(bbox.minpt == self._volume.bounds.minpt))
                and (not np.any(bbox.maxpt == self._volume.bounds.maxpt))):
            return data, Vec(0, 0, 0)

        shape = [int(s) for s in data.shape]
        offset = [0, 0, 0, 0]
        for i in range(3):
            if bbox.minpt[i] == self._volume.voxel_offset[i]:
                offset[i] += 1
                shape[i] += 1
            if bbox.maxpt[i] == self._volume.bounds.maxpt[i]:
                shape[i] += 1

        slices = tuple(
            slice(offset[i], offset[i] + data.shape[i]) for i in range(3))

        mirror_data = np.zeros(shape, dtype=data.dtype, order="F")
        mirror_data[slices[0], slices[1], slices[2]] = data
        if offset[0]:
            mirror_data[0, :, :] = 0
        if offset[1]:
            mirror_data[:, 0, :] = 0
        if offset[2]:
            mirror_data[:, :, 0] = 0
        return mirror_data, Vec(*offset[:3])

    def get_mesh_dir(self):
        if self.options['mesh_dir'] is not None:
            return self.options['mesh_dir']
        elif 'mesh' in self._volume.info:
            return self._volume.info['mesh']
        raise ValueError("The mesh destination is not present in the info file.")

    def _global_voxel_counts(self):
        """The dataset's voxel_counts.im sidecar (mesh.py:325-345), parsed
        once per process and path."""
        from .voxel_counts import voxel_counts_sidecar
        name = voxel_counts_sidecar(self._volume.key)
        path = f"{self._volume.cloudpath}/{name}"
        counts = _voxel_counts_cache.get(path)
        if counts is None:
            buf = CloudFiles(self._volume.cloudpath).get(name)
            if buf is None:
                raise FileNotFoundError(
                    f"Cannot apply global dust threshold without {path}")
            from ..formats.intmap import IntMap
            counts = _voxel_counts_cache[path] = IntMap(buf)
        return counts

    def _remove_dust(self, data, dust_threshold):
        """The chunk-local threshold on the host (mesh.py:317-320)."""
        if not dust_threshold:
            return data
        segids, pxct = fastremap_np.unique(data, return_counts=True)
        dust_segids = [int(sid) for sid, ct in zip(segids, pxct)
                       if ct < int(dust_threshold) and sid != 0]
        return fastremap_np.mask(data, dust_segids, in_place=True)

    def _remap(self, data):
        if self.options['remap_table'] is None:
            return data
        remap_table = dict(self.options['remap_table'])  # ints already
        remap_table[0] = 0
        data = fastremap_np.mask_except(
            data, list(remap_table.keys()), in_place=True)
        return fastremap_np.remap(data, remap_table, in_place=True)

    def _global_shift(self, left_bound_offset):
        """Chunk-local nm -> global nm (mesh.py:434-435), three f32."""
        resolution = self._volume.resolution
        offset = (self._bounds.minpt - self.options['low_padding']).astype(np.float32)
        return ((offset - np.asarray(left_bound_offset, dtype=np.float32))
                * np.asarray(resolution, dtype=np.float32))

    def _create_mesh_binary(self, mesh: Mesh, left_bound_offset):
        return encode_fragment(
            mesh, self._global_shift(left_bound_offset),
            self.options['encoding'],
            getattr(self, 'draco_encoding_settings', None))

    def _upload_batch(self, mesh_binaries, bbox: Bbox):
        """Sharded fragment output (reference mesh.py:385-397): all the
        chunk's meshes in ONE MapBuffer file
        "{mesh_dir}/{bbox.to_filename()}.frags", consumed per label by
        the sharded multires merge (multires.py:425). The reference
        compresses values with brotli ("br"); offline that downgrades to
        gzip inside our MapBuffer restatement (formats/mapbuffer.py,
        DESIGN.md §7)."""
        from ..formats.mapbuffer import MapBuffer
        frag_path = self.options['frag_path'] or self.layer_path
        cf = CloudFiles(frag_path)
        mbuf = MapBuffer(
            {int(k): v for k, v in mesh_binaries.items()}, compress="br")
        cf.put(
            f"{self._mesh_dir}/{bbox.to_filename()}.frags",
            mbuf.tobytes(),
            compress=None,
            content_type="application/x.mapbuffer",
            cache_control=False,
        )

    def _upload_individuals(self, mesh_binaries, generate_manifests):
        cf = CloudFiles(self.layer_path)
        content_type = ("model/x.draco"
                        if self.options["encoding"] == "draco"
                        else "model/mesh")  # mesh.py:403-406
        cf.puts(
            ((f"{self._mesh_dir}/{segid}:{self.options['lod']}:"
              f"{self._bounds.to_filename()}", binary)
             for segid, binary in mesh_binaries.items()),
            compress=self._encoding_to_compression_dict[self.options['encoding']],
            cache_control=self.options['cache_control'],
            content_type=content_type,
        )
        if generate_manifests:
            cf.put_jsons(
                ((f"{self._mesh_dir}/{segid}:{self.options['lod']}",
                  {"fragments": [
                      f"{segid}:{self.options['lod']}:"
                      f"{self._bounds.to_filename()}"]})
                 for segid in mesh_binaries),
                compress=None,
                cache_control=self.options['cache_control'],
            )

    def _upload_spatial_index(self, bbox: Bbox, mesh_bboxes: dict):
        # mirrors mesh.py:452-464: filename precision comes from the mesh
        # info's spatial_index metadata (cloudvolume's
        # vol.mesh.spatial_index.precision); absent → integer naming.
        cf = CloudFiles(self.layer_path)
        mesh_info = cf.get_json(f"{self._mesh_dir}/info") or {}
        precision = (mesh_info.get('spatial_index') or {}).get('precision', None)
        resolution = np.asarray(self._volume.resolution, dtype=np.int64)
        nm_bbox = Bbox(bbox.minpt * resolution, bbox.maxpt * resolution)
        cf.put_json(
            f"{self._mesh_dir}/{nm_bbox.to_filename(precision)}.spatial",
            {str(k): v for k, v in mesh_bboxes.items()},
            compress=self.options['compress'],
        )


# ----------------------------------------------------------------------
# Stage-2 manifest tasks (reference mesh.py:624-724): list per-chunk mesh
# fragments and write "{segid}:{lod}" JSON manifests so Neuroglancer knows
# which fragments to fetch for a segid. Pure string/IO postprocess.

import re as _re
from collections import defaultdict as _defaultdict


def _write_manifests(layer_path: str, lod: int, mesh_dir, prefix=None):
    """Group the mesh dir's fragment files of `lod` (those starting with
    `prefix`, if given) by segid and write one {"fragments": [...]}
    manifest per segid."""
    cf = CloudFiles(layer_path)
    info = cf.get_json('info')
    if mesh_dir is None and info and 'mesh' in info:
        mesh_dir = info['mesh']

    segids = _defaultdict(list)
    regexp = _re.compile(r'(\d+):(\d+):')
    for name in cf.list(prefix=f"{mesh_dir}/" if prefix is None
                        else cf.join(mesh_dir, prefix)):
        filename = name.split("/")[-1]
        matches = _re.search(regexp, filename)
        if not matches:
            continue
        segid, mlod = int(matches.group(1)), int(matches.group(2))
        if mlod != lod:
            continue
        segids[segid].append(filename)

    cf.put_jsons(
        (f"{mesh_dir}/{segid}:{lod}", {"fragments": frags})
        for segid, frags in segids.items())


def MeshManifestFilesystemTask(layer_path: str, lod: int = 0,
                               mesh_dir=None):
    """Mirror of the reference's filesystem manifest task
    (mesh.py:624-670): scan the mesh dir, group fragment files by segid,
    write {"fragments": [...]} manifests."""
    _write_manifests(layer_path, lod, mesh_dir)


def MeshManifestPrefixTask(layer_path: str, prefix: str, lod: int = 0,
                           mesh_dir=None):
    """Mirror of the reference's prefix-parallelized manifest task
    (mesh.py:672-724)."""
    _write_manifests(layer_path, lod, mesh_dir, prefix)


def TransferMeshFilesTask(src: str, dest: str, prefix: str,
                          mesh_dir=None):
    """Copy mesh files between layers (reference mesh.py:726-739)."""
    from ..volume import PrecomputedVolume
    cv_src = PrecomputedVolume(src)
    cv_dest = PrecomputedVolume(dest)
    sdir = mesh_dir or cv_src.info.get('mesh', 'mesh')
    ddir = mesh_dir or cv_dest.info.get('mesh', sdir)
    cf_src = CloudFiles(f"{src.rstrip('/')}/{sdir}")
    cf_dest = CloudFiles(f"{dest.rstrip('/')}/{ddir}")
    for name in cf_src.list(prefix=prefix):
        data = cf_src.get(name)
        if data is not None:
            cf_dest.put(name, data)


def DeleteMeshFilesTask(cloudpath: str, prefix: str, mesh_dir=None):
    """Delete mesh files under a prefix (reference mesh.py:741-749)."""
    from ..volume import PrecomputedVolume
    cv = PrecomputedVolume(cloudpath)
    mdir = mesh_dir or cv.info.get('mesh', 'mesh')
    cf = CloudFiles(f"{cloudpath.rstrip('/')}/{mdir}")
    cf.delete(list(cf.list(prefix=prefix)))
