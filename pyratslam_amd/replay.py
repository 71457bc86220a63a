"""Bag replay of the reference's ROS node (config 5), headless.

``RatslamReplay`` is ``RatslamRos`` (``/root/reference/ratslam/ros_simulate.py:45-170``)
with the rospy plumbing replaced by a deterministic event loop over a recorded
bag: the same constants (POSE_SIZE, IM_SIZE, ranges, steps, MATCH_THRESHOLD,
ODOM_FREQ, :31-41), the same start (inject 1 at the grid midpoint, :56-57) and
the same callbacks:

* ``odom_callback`` (:125-129) queues a twist when |linear.x| or |angular.z|
  exceeds 0.001;
* ``update_posecells`` (:134-146) steps the network with (x / ODOM_FREQ,
  z / ODOM_FREQ), reads the peak cell and advances the experience map;
* ``vis_callback`` (:98-113) converts the frame to mono8, matches it against the
  view templates at the current peak cell and records the template index
  (optionally feeding the match back: the reference's commented-out
  ``pcn.inject(e, template.location())``, :107-108).

Interleaving: the ROS node drains the twist queue on its main thread while the
image callback runs on a subscriber thread; the replay fixes the order the node
takes when its main loop keeps up -- messages in bag order, every queued twist
applied before the next frame is matched.  Consecutive twists are applied with
one ``PoseCellNetwork.run`` (one host round trip), which gives the same states
and peaks as one ``update`` each.

Outputs (the node's published topics): ``pc_max`` per update, ``em_points``
(``navbot/experiencemap``, :142-146) and ``template_index`` per frame
(``navbot/templatematches``, :110-113).

``use_visual_odometry=True`` is the node's ``USE_VISUAL_ODOMETRY`` mode (:81, :90,
:119-122, :163-165): odometry messages are ignored, ``vis_callback`` matches the
frame at the current peak and then queues ``vo.update(im)``, and that delta is
applied, undivided and unfiltered, right after its frame.  ``replay_frames`` is the
same pipeline over an array of frames, batched on the GPU.

``python -m pyratslam_amd.replay --bag FILE`` replays a bag;
``--synthetic N`` writes and replays a synthetic one (``synthetic.ros_stream``);
``--visual-odometry`` replays either from the camera alone; ``--loop-closure`` keeps a
``LinkedExperienceMap`` (every matched frame goes to ``em.on_template``, which links the
experiences and relaxes the map on the GPU) in place of the dead-reckoned ``ExperienceMap``;
``--subcell-peak`` also records the sub-cell pose of every update (``pc_pose``: the activity
packet's circular centroid, ``PoseCellNetwork.update_pose`` / ``run(poses=True)``), while the
view templates, the feedback injection and both maps still receive the integer peak cell;
``--window K`` (``RatslamReplay(window=K)``) matches K frames with one ``match_batch`` and steps
the twists between them with one ``run``, the feedback injections inside it
(``run(injections=...)``), with the outputs of the frame-by-frame loop;
``--view-shift [--view-fov RAD]`` (``RatslamReplay(view_shift=True, view_fov=RAD)``) stores the
view templates column-major, records the row offset of every match (``view_offset``) and hands
it to the linked map as the angle the place is seen turned by.
"""
import argparse
import json
import math
import sys
import time
from collections import deque

import numpy as np

from . import rosbag
from .experience_map import ExperienceMap

# ros_simulate.py:31-41
POSE_SIZE = (21, 21, 36)
IM_SIZE = (256, 256)
X_RANGE = (32, 96)
Y_RANGE = (32, 96)
X_STEP = 2
Y_STEP = 2
MATCH_THRESHOLD = 45000
ODOM_FREQ = 10
ODOM_TOPIC = 'navbot/odom'
IMAGE_TOPIC = 'navbot/camera/image'


def window_boundaries(messages, odom_freq=ODOM_FREQ):
    """The window scheduler's first half, a pure function of a window's messages --
    ``('odom', twist)`` with ``twist.linear`` / ``twist.angular``, or ``('image', frame)`` --
    to ``(steps, bounds)``: the (vtrans, vrot) of every twist the node would queue
    (``odom_callback``'s 0.001 filter, ``drain``'s division), and for each frame its boundary,
    the number of steps applied before the frame is matched."""
    steps, bounds = [], []
    for kind, msg in messages:
        if kind == 'odom':
            if abs(msg.linear[0]) > 0.001 or abs(msg.angular[2]) > 0.001:
                steps.append((msg.linear[0] / odom_freq, msg.angular[2] / odom_freq))
        else:
            bounds.append(len(steps))
    return steps, bounds


def injection_kinds(template_index, known):
    """... and its second half: the injection of each frame of a window (or batch) from the
    frames' template indices and the number of templates ``known`` before it:
    ``('stored', t)`` for a template that existed, ``('peak',)`` for the frame that creates
    one (it is stored, and fed back, at the peak of that moment) and ``('same', j)`` for a
    later frame that matches the template frame j of this window created."""
    kinds, creator = [], {}
    for j, t in enumerate(int(t) for t in template_index):
        if t < known:
            kinds.append(('stored', t))
        elif t in creator:
            kinds.append(('same', creator[t]))
        else:
            creator[t] = j
            kinds.append(('peak',))
    return kinds


class RatslamReplay:
    """``RatslamRos`` driven by recorded messages.

    ``pcn`` / ``vts`` / ``em``: objects with the reference's APIs; by default the
    MI355X ``PoseCellNetwork`` and ``ViewTemplates`` of this package (any other
    implementation with the same API -- the CPU oracle, the reference itself --
    can be dropped in, which is how parity is checked)."""

    def __init__(self, pose_size=POSE_SIZE, im_size=IM_SIZE, x_range=X_RANGE, y_range=Y_RANGE,
                 x_step=X_STEP, y_step=Y_STEP, match_threshold=MATCH_THRESHOLD,
                 odom_freq=ODOM_FREQ, feedback_energy=None, pcn=None, vts=None, em=None,
                 device=0, precision='float32', batch=True, publish=False,
                 use_visual_odometry=False, vo=None, subcell_peak=False, window=1, vt_metric='wrapped',
                 view_shift=False, view_fov=None, vt_normalise=None):
        """``vt_normalise``: None, or ``(radius, gain)``: the view templates are patch-normalised
        on the GPU (``ViewTemplates(normalise=...)``), against a change of exposure between visits.
        ``view_shift``: the view templates are stored column-major (``shift_axis='cols'``) and
        every match's row offset is recorded (``results()['view_offset']``) and passed to a
        linked map as ``rel_rad = offset * x_step * view_fov / im_width``: one template row is
        ``x_step`` image columns, and a frame of ``im_width`` columns spans ``view_fov``, the
        camera's horizontal field of view in radians.  Its sign is the camera's handedness:
        positive where a larger heading moves the view towards larger image columns, as in
        ``synthetic.ros_stream`` (+pi/2: a larger heading gives a positive offset there)."""
        from .view_templates import _normalise_arg
        vt_normalise = _normalise_arg(vt_normalise)     # (a ValueError before anything is created)
        # publish: the node's per-step work in full -- every update reads the whole
        # .posecells volume, as ros_simulate.py:140-145 does to publish it -- so steps
        # go one by one (no batched run()) and the network exports eagerly
        self.publish = publish
        if pcn is None:
            from .posecell_network import PoseCellNetwork
            pcn = PoseCellNetwork(shape=pose_size, precision=precision, device=device,
                                  readback='eager' if publish else 'lazy')
        self.view_shift = bool(view_shift)
        if self.view_shift and view_fov is None:
            raise ValueError('view_shift needs view_fov, the camera\'s horizontal field of view in radians')
        if vts is None:
            from .view_templates import ViewTemplates
            shift = {'shift_axis': 'cols', 'offsets': True} if self.view_shift else {}
            vts = ViewTemplates(x_range=x_range, y_range=y_range, x_step=x_step, y_step=y_step,
                                im_x=im_size[0], im_y=im_size[1], match_threshold=match_threshold,
                                device=device, metric=vt_metric, normalise=vt_normalise, **shift)
        elif self.view_shift and not (getattr(vts, 'offsets', False)
                                      and getattr(vts, 'shift_axis', 'rows') == 'cols'):
            raise ValueError("view_shift needs view templates built with shift_axis='cols', offsets=True")
        elif getattr(vts, 'metric', vt_metric) != vt_metric:
            raise ValueError('vt_metric=%r, but the view templates passed in score by %r'
                             % (vt_metric, vts.metric))
        elif getattr(vts, 'normalise', vt_normalise) != vt_normalise:
            raise ValueError('vt_normalise=%r, but the view templates passed in normalise by %r'
                             % (vt_normalise, vts.normalise))
        # the metric of the default uint8 library ('wrapped': the reference's numpy arithmetic on
        # mono8 frames; 'sad': true |T - Q|, for two-sided camera noise -- with a threshold of
        # its own, the shipped 45000 sits on the wrapped metric's noise floor)
        self.vt_metric = vt_metric
        self.vt_normalise = vt_normalise
        self.pcn, self.vts = pcn, vts
        # radians per template row, and the offsets of the frames so far
        self.rad_per_row = float(x_step) * float(view_fov) / float(im_size[1]) if self.view_shift else 0.0
        self.view_offset = []
        self.em = em if em is not None else ExperienceMap()
        self._em_links = hasattr(self.em, 'on_template')   # (LinkedExperienceMap)
        self.odom_freq = odom_freq
        self.feedback_energy = feedback_energy
        self.batch = batch and hasattr(pcn, 'run') and not publish
        # run(injections=...): the feedback inside a batched run (the oracle has none)
        self._run_injects = self.batch and _takes_injections(pcn)
        # window: frames matched, and their twists stepped, per batched call of replay_events /
        # replay_bag (1: the per-frame loop)
        if int(window) != window or window < 1:
            raise ValueError('window must be a positive integer, got %r' % (window,))
        self.window = int(window)
        self.published = 0   # .posecells volumes read (publish=True)
        self.twist_data = deque()
        # USE_VISUAL_ODOMETRY (ros_simulate.py:81, 90): no odometry subscription, every
        # frame through vo.update(im); vo = any object with update() (NumpyVisualOdometer)
        self.use_visual_odometry = bool(use_visual_odometry)
        if self.use_visual_odometry and vo is None:
            from .visual_odometer import SimpleVisualOdometer
            vo = SimpleVisualOdometer(device=device)
        self.vo = vo
        self.vis_odom_data = deque()
        self.deltas = []     # the visual deltas, one (vtrans, vrot) per frame
        # ros_simulate.py:56-57 (Python-2 int / 2, then math.floor)
        self.pcn.inject(1, tuple(int(math.floor(s // 2)) for s in pose_size))
        self.pc_max, self.em_points, self.template_index = [], [], []
        # the sub-cell pose of every update, recorded next to pc_max (results()['pc_pose'])
        self.subcell_peak = bool(subcell_peak)
        self.pc_pose = []

    # -- callbacks ---------------------------------------------------------------
    def odom_callback(self, twist):
        """ros_simulate.py:125-129 (not subscribed under visual odometry, :81)."""
        if self.use_visual_odometry:
            return
        if abs(twist.linear[0]) > 0.001 or abs(twist.angular[2]) > 0.001:
            self.twist_data.append(twist)

    def vis_callback(self, im):
        """ros_simulate.py:98-113 (after imgmsg_to_cv(data, "mono8"))."""
        pc_max = self.pcn.get_pc_max()
        template_match = self.vts.match(input=im, pc_x=pc_max[0], pc_y=pc_max[1], pc_th=pc_max[2])
        self.template_index.append(int(template_match.get_index()))
        rel = self._view_rel(1)
        if self._em_links:   # a linked map learns which place the frame was recognised as
            self._on_template(self.template_index[-1], rel[0])
        if self.feedback_energy:
            self.pcn.inject(self.feedback_energy, tuple(template_match.location()))
        if self.use_visual_odometry:   # ros_simulate.py:119-122
            delta = self.vo.update(im)
            self.deltas.append((float(delta[0]), float(delta[1])))
            self.vis_odom_data.append(delta)

    def _view_rel(self, n):
        """``view_shift``: record the offsets of the ``n`` frames just matched
        (``vts.last_offsets``) and return their ``rel_rad``; all zero when off."""
        if not self.view_shift:
            return [0.0] * n
        off = [int(o) for o in self.vts.last_offsets]
        assert len(off) == n, (len(off), n)
        self.view_offset.extend(off)
        return [o * self.rad_per_row for o in off]

    def _on_template(self, index, rel):
        if self.view_shift:
            self.em.on_template(index, rel)
        else:
            self.em.on_template(index)

    def update_posecells(self, vtrans, vrot):
        """ros_simulate.py:134-146 (publishing reduced to recording; with publish=True
        the volume is read as the node reads it to publish, :140)."""
        if self.subcell_peak:
            self.pc_pose.append(tuple(self.pcn.update_pose((vtrans, vrot))))
        else:
            self.pcn.update((vtrans, vrot))
        self._record(vtrans, vrot, self.pcn.get_pc_max())
        if self.publish:
            pc = self.pcn.posecells
            self.published += pc.size

    def _record(self, vtrans, vrot, pc_max):
        pc_max = tuple(int(v) for v in pc_max)
        self.em.update(vtrans, vrot, pc_max)
        self.pc_max.append(pc_max)
        self.em_points.append(tuple(float(v) for v in self.em.get_current_point()))

    def drain(self):
        """The main loop's queue drain (ros_simulate.py:156-166): twists divided by
        ODOM_FREQ, visual deltas as they are (no 0.001 filter, no division)."""
        steps = []
        while self.twist_data:
            twist = self.twist_data.popleft()
            steps.append((twist.linear[0] / self.odom_freq, twist.angular[2] / self.odom_freq))
        while self.vis_odom_data:
            vtrans, vrot = self.vis_odom_data.popleft()
            steps.append((float(vtrans), float(vrot)))
        if not steps:
            return
        if self.batch:
            maxes = self._run(np.array(steps, dtype=np.float64))
            for (vt, vr), m in zip(steps, maxes):
                self._record(vt, vr, m)
        else:
            for vt, vr in steps:
                self.update_posecells(vt, vr)

    def _run(self, odometry, injections=None):
        """``pcn.run``; with ``subcell_peak`` the poses come back with the peaks and are recorded.
        With ``injections``: ``(maxes, cells)``."""
        kw = {} if injections is None else {'injections': injections}
        if not self.subcell_peak:
            return self.pcn.run(odometry, **kw)
        maxes, poses, *cells = self.pcn.run(odometry, poses=True, **kw)
        self.pc_pose.extend(tuple(float(v) for v in p) for p in poses)
        return maxes if injections is None else (maxes, cells[0])

    def _feedback_injections(self, kinds, bounds):
        """``injection_kinds`` as ``run(injections=...)``: frame j injects at its boundary."""
        where = {'stored': lambda t: tuple(self.vts.templates[t].location()),
                 'peak': lambda: self.pcn.AT_PEAK, 'same': lambda j: ('same', j)}
        return [(b, self.feedback_energy, where[k[0]](*k[1:])) for k, b in zip(kinds, bounds)]

    def _windowed(self):
        """Whether replay_events / replay_bag go window by window (else the per-frame loop)."""
        return (self.window > 1 and self._run_injects and not self.use_visual_odometry
                and hasattr(self.vts, 'match_batch') and getattr(self.vts, 'nranks', 1) == 1)

    def _replay_messages(self, messages):
        """``('odom', twist)`` / ``('image', frame)`` messages in order: the per-frame loop, or
        windows of up to ``window`` frames with the twists between them."""
        if not self._windowed():
            for kind, msg in messages:
                if kind == 'odom':
                    self.odom_callback(msg)
                else:
                    self.drain()
                    self.vis_callback(msg)
                    if self.use_visual_odometry:   # a visual delta is applied right after its frame
                        self.drain()
            self.drain()
            return self
        self.drain()
        pending, frames = [], 0
        for m in messages:
            pending.append(m)
            frames += m[0] != 'odom'
            if frames == self.window:
                self._replay_window(pending)
                pending, frames = [], 0
        self._replay_window(pending)
        return self

    def _replay_window(self, messages):
        """One window: one ``match_batch`` of its frames with placeholder cells, one ``run`` of
        all its steps (with feedback, the frames' injections at their boundaries), the new
        templates' cells filled in, then the records in message order."""
        steps, bounds = window_boundaries(messages, self.odom_freq)
        images = [m[1] for m in messages if m[0] != 'odom']
        if not steps and not images:
            return
        known = len(self.vts.templates)
        matched = self.vts.match_batch(images, [(0, 0, 0)] * len(images)) if images else []
        index = [int(t.get_index()) for t in matched]
        rel = self._view_rel(len(index)) if images else []
        kinds = injection_kinds(index, known)
        od = np.array(steps, dtype=np.float64).reshape(-1, 2)
        if self.feedback_energy and images:
            maxes, cells = self._run(od, self._feedback_injections(kinds, bounds))
        else:
            # a template created in front of the window's first step is stored at the peak now
            start = (self.pcn.get_pc_max() if any(k == ('peak',) and b == 0 for k, b in zip(kinds, bounds))
                     else None)
            maxes = self._run(od) if steps else []
            cells = [start if b == 0 else maxes[b - 1] for b in bounds]
        for t, k, cell in zip(matched, kinds, cells):
            if k == ('peak',):
                t.pc_x, t.pc_y, t.pc_th = (int(v) for v in cell)
        frame = 0
        for s in range(len(steps) + 1):
            while frame < len(bounds) and bounds[frame] == s:
                self.template_index.append(index[frame])
                if self._em_links:
                    self._on_template(index[frame], rel[frame])
                frame += 1
            if s < len(steps):
                self._record(steps[s][0], steps[s][1], maxes[s])

    # -- drivers -----------------------------------------------------------------
    def replay_events(self, events):
        """``synthetic.ros_stream`` events (already decoded)."""
        return self._replay_messages(('odom', rosbag.Twist(ev[2], ev[3])) if ev[0] == 'odom' else ('image', ev[2])
                                     for ev in events)

    def replay_bag(self, path, odom_topic=ODOM_TOPIC, image_topic=IMAGE_TOPIC):
        """Messages of a bag in order; odometry from nav_msgs/Odometry (or a bare
        geometry_msgs/Twist), frames from sensor_msgs/Image."""
        o, i = odom_topic.lstrip('/'), image_topic.lstrip('/')
        def messages():
            for m in rosbag.read_bag(path, topics={o, i}):
                if m.topic.lstrip('/') == o:
                    yield 'odom', (rosbag.decode_twist(m.data) if m.type == 'geometry_msgs/Twist' else
                                   rosbag.decode_odometry_twist(m.data))
                else:
                    yield 'image', rosbag.image_to_mono8(rosbag.decode_image(m.data))
        return self._replay_messages(messages())

    def replay_frames(self, frames, batch=64):
        """The camera-only pipeline (``use_visual_odometry=True``) over a uint8
        ``(n, im_h, im_w)`` array, batched: each batch is uploaded once into a
        ``DeviceBuffer``; ``vo.run`` on the buffer gives its deltas, ``pcn.run(deltas)``
        its peaks, and ``vts.match_frames`` matches frame i at the peak after deltas
        0..i-1 (the last peak carries over from the batch before).  Without feedback
        that is exactly the per-frame order -- match at the current peak, then the
        frame's delta, then the step.  With ``feedback_energy`` the match changes the
        state the next step starts from, but not the other way round (a match depends on
        the frames and the library only): the batch is matched with placeholder cells,
        then stepped by one ``pcn.run(deltas, injections=...)`` with frame i's injection in
        front of step i -- at the stored cell of a template that existed, at the peak of that
        moment for the frame that creates one, at the same cell for a later frame of the batch
        that matches it -- and the new templates take the cells their injections resolved to.
        With a drop-in ``vo`` / ``vts`` / ``pcn`` that has no batched form, the frames go one
        by one through ``vis_callback``."""
        if not self.use_visual_odometry:
            raise ValueError('replay_frames is the camera-only pipeline: construct with '
                             'use_visual_odometry=True')
        f = np.asarray(frames)
        if f.dtype != np.uint8:
            raise TypeError('replay_frames takes uint8 frames (mono8); got %s' % f.dtype)
        if f.ndim != 3:
            raise ValueError('frames must be (n, im_h, im_w), got shape %r' % (f.shape,))
        from .visual_odometer import SimpleVisualOdometer
        batched = ((not self.feedback_energy or self._run_injects) and self.batch and batch > 1
                   and isinstance(self.vo, SimpleVisualOdometer)
                   and hasattr(self.vts, 'match_frames') and getattr(self.vts, 'nranks', 1) == 1)
        if not batched:
            for im in f:
                self.vis_callback(im)
                self.drain()
            return self
        if f.shape[0] == 0:
            return self
        mask = getattr(self.vts, 'mask', None)
        if mask is not None and f.shape[1:] != mask.shape:
            raise ValueError('frame shape %r does not match the mask %r' % (f.shape[1:], mask.shape))
        from . import _lib
        f = np.ascontiguousarray(f)
        self.drain()
        self.vo.setup(f.shape[1:])
        buf = _lib.DeviceBuffer(int(batch) * f[0].size, device=self.vo.device)
        try:
            for i0 in range(0, f.shape[0], int(batch)):
                chunk = f[i0:i0 + int(batch)]
                n = chunk.shape[0]
                buf.upload(chunk)
                deltas = self.vo.run((n, buf))
                if self.feedback_energy:
                    # the match does not depend on the pose cells: placeholder cells, then one
                    # run with frame i's injection in front of step i, and the new templates'
                    # cells from what their at-peak injections resolved to
                    known = len(self.vts.templates)
                    idx, _, new = self.vts.match_frames((n, buf), None)
                    kinds = injection_kinds(idx, known)
                    maxes, cells = self._run(deltas, self._feedback_injections(kinds, range(n)))
                    for j in np.flatnonzero(new):
                        t = self.vts.templates[int(idx[j])]
                        t.pc_x, t.pc_y, t.pc_th = (int(v) for v in cells[j])
                else:
                    peak = tuple(int(v) for v in self.pcn.get_pc_max())
                    maxes = self._run(deltas)
                    pcs = [peak] + [tuple(int(v) for v in m) for m in maxes[:-1]]
                    idx, _, _ = self.vts.match_frames((n, buf), pcs)
                self.template_index.extend(int(j) for j in idx)
                rel = self._view_rel(n)
                for (vt, vr), m, j, rr in zip(deltas, maxes, idx, rel):
                    if self._em_links:   # the frame's match, then its step: the per-frame order
                        self._on_template(int(j), rr)
                    self.deltas.append((float(vt), float(vr)))
                    self._record(float(vt), float(vr), m)
        finally:
            buf.close()
        return self

    def results(self):
        return {**({'pc_pose': np.array(self.pc_pose, dtype=np.float64).reshape(-1, 3)}
                   if self.subcell_peak else {}),
                'pc_max': np.array(self.pc_max, dtype=np.int64).reshape(-1, 3),
                'em_points': np.array(self.em_points, dtype=np.float64).reshape(-1, 2),
                'template_index': np.array(self.template_index, dtype=np.int64),
                **({'view_offset': np.array(self.view_offset, dtype=np.int64)} if self.view_shift else {}),
                'templates': len(self.vts.templates)}


def _takes_injections(pcn):
    """Whether ``pcn.run`` takes ``injections`` (PoseCellNetwork's; a drop-in may not)."""
    import inspect
    try:
        return 'injections' in inspect.signature(pcn.run).parameters
    except (TypeError, ValueError):
        return False


def sharded_templates(d, device, host_reduce=False, x_range=X_RANGE, y_range=Y_RANGE, x_step=X_STEP,
                      y_step=Y_STEP, im_size=IM_SIZE, match_threshold=MATCH_THRESHOLD, metric='wrapped',
                      normalise=None):
    """The view-template library sharded over the ranks of ``d`` (a dist.Dist):
    template g on rank g % N, one RCCL allreduce(min) per match (or the host
    reducer of the control plane with ``host_reduce``, for several ranks on one
    GPU)."""
    from .view_templates import ShardedViewTemplates
    if host_reduce:
        return ShardedViewTemplates(x_range, y_range, x_step, y_step, im_size[0], im_size[1],
                                    match_threshold, d.rank, d.world, reducer=d.min_keys, device=device,
                                    metric=metric, normalise=normalise)
    uid = d.bcast_bytes(ShardedViewTemplates.unique_id() if d.rank == 0 else None)
    return ShardedViewTemplates(x_range, y_range, x_step, y_step, im_size[0], im_size[1],
                                match_threshold, d.rank, d.world, reducer='rccl', unique_id=uid,
                                device=device, metric=metric, normalise=normalise)


VT_NORMALISE_GAIN = 32   # --vt-normalise R: the gain when only the radius is given


def parse_vt_normalise(text):
    """``R`` or ``R,G`` of ``--vt-normalise`` -> ``(radius, gain)``."""
    from .view_templates import _normalise_arg
    parts = text.split(',')
    try:
        if len(parts) not in (1, 2):
            raise ValueError(text)
        value = (int(parts[0]), int(parts[1]) if len(parts) == 2 else VT_NORMALISE_GAIN)
        return _normalise_arg(value)
    except ValueError as e:
        raise argparse.ArgumentTypeError('expected R or R,G with R in 1..7 and G in 1..127 (%s)' % e)


def build_parser():
    """The command line of ``python -m pyratslam_amd.replay``."""
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--bag', help='ROS 1 bag with navbot/odom and navbot/camera/image')
    src.add_argument('--synthetic', type=int, metavar='N', help='replay N synthetic odometry+frame pairs')
    ap.add_argument('--device', type=int, default=None, help='default: LOCAL_RANK')
    ap.add_argument('--precision', default='float32')
    ap.add_argument('--feedback', type=float, default=None,
                    help='inject this energy at each matched template (ros_simulate.py:107-108)')
    ap.add_argument('--gpus', type=int, default=1,
                    help='ranks (launched here, or by torch.distributed.run): the template '
                         'library is sharded over them, the pose cells are replicated')
    ap.add_argument('--visual-odometry', action='store_true',
                    help='camera-only replay (USE_VISUAL_ODOMETRY, ros_simulate.py:81): odometry '
                         'messages are ignored, every frame goes through SimpleVisualOdometer; '
                         'each rank runs its own odometer replica')
    ap.add_argument('--loop-closure', action='store_true',
                    help='keep a LinkedExperienceMap: one experience per view template, links '
                         'from odometry, relaxed on the GPU after every frame; each rank keeps '
                         'its own replica')
    ap.add_argument('--exp-loops', type=int, default=None, metavar='N',
                    help='relaxation sweeps per frame under --loop-closure (default 100)')
    ap.add_argument('--subcell-peak', action='store_true',
                    help='record the sub-cell pose of every update (pc_pose): the activity '
                         'packet\'s circular centroid, computed on the GPU behind each step')
    ap.add_argument('--window', type=int, default=1, metavar='K',
                    help='match K frames and step the twists between them per batched call '
                         '(odometry mode; 1: frame by frame)')
    ap.add_argument('--view-shift', action='store_true',
                    help='store the view templates column-major and use the row offset of every '
                         'match as the angle the place is seen turned by (view_offset; with '
                         '--loop-closure it corrects the closure links); one GPU')
    ap.add_argument('--view-fov', type=float, default=None, metavar='RAD',
                    help='the camera\'s horizontal field of view in radians under --view-shift, '
                         'signed by its handedness (default pi/2, synthetic.ros_stream\'s camera)')
    ap.add_argument('--host-reduce', action='store_true',
                    help='combine the ranks\' keys on the host (several ranks on one GPU)')
    ap.add_argument('--vt-metric', choices=('wrapped', 'sad'), default='wrapped',
                    help='score of the uint8 view templates: "wrapped" is the reference\'s numpy '
                         'arithmetic on mono8 frames, sum((T - Q) mod 256), where a pixel one grey '
                         'level above its template scores 255; "sad" is the true sum of |T - Q|, '
                         'for cameras with two-sided noise.  Choose --match-threshold with it')
    ap.add_argument('--vt-normalise', type=parse_vt_normalise, default=None, metavar='R[,G]',
                    help='patch-normalise the uint8 view templates on the GPU, against a change of '
                         'exposure between visits: every pixel in units of the standard deviation '
                         'of its (2R+1)^2 neighbourhood, G grey levels per unit around 128 (R in '
                         '1..7, G in 1..127, default %d).  Choose --match-threshold with it'
                         % VT_NORMALISE_GAIN)
    ap.add_argument('--match-threshold', type=float, default=MATCH_THRESHOLD, metavar='T',
                    help='a frame whose best score exceeds T becomes a new template (default %d, '
                         'the reference\'s, which sits on the wrapped metric\'s noise floor: under '
                         '--vt-metric sad, 300 frames of the synthetic stream make a single '
                         'template with it, and 61 with 2048, 4 per window pixel)' % MATCH_THRESHOLD)
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.exp_loops is not None and not args.loop_closure:
        ap.error('--exp-loops needs --loop-closure')
    if args.view_fov is not None and not args.view_shift:
        ap.error('--view-fov needs --view-shift')
    if args.view_shift and args.gpus > 1:
        ap.error('--view-shift needs an unsharded template library (--gpus 1)')
    from . import launch
    if args.gpus > 1 and not launch.under_launcher():
        return launch.spawn(args.gpus, ['-m', 'pyratslam_amd.replay'] + list(
            sys.argv[1:] if argv is None else argv))
    from .dist import Dist
    d = Dist(args.gpus)
    dev = d.local if args.device is None else args.device
    vts = (sharded_templates(d, dev, args.host_reduce, match_threshold=args.match_threshold,
                             metric=args.vt_metric, normalise=args.vt_normalise) if d.world > 1 else None)
    em = None
    if args.loop_closure:
        from .linked_experience_map import EXP_LOOPS, LinkedExperienceMap
        em = LinkedExperienceMap(exp_loops=EXP_LOOPS if args.exp_loops is None else args.exp_loops,
                                 device=dev)
    r = RatslamReplay(device=dev, precision=args.precision, feedback_energy=args.feedback, vts=vts,
                      use_visual_odometry=args.visual_odometry, em=em, subcell_peak=args.subcell_peak,
                      window=args.window, vt_metric=args.vt_metric, vt_normalise=args.vt_normalise,
                      match_threshold=args.match_threshold,
                      view_shift=args.view_shift,
                      view_fov=(math.pi / 2 if args.view_fov is None else args.view_fov) if args.view_shift else None)
    d.barrier()
    t0 = time.perf_counter()
    if args.bag:
        r.replay_bag(args.bag)
    else:
        from . import synthetic
        r.replay_events(synthetic.ros_stream(args.synthetic))
    dt = d.max(time.perf_counter() - t0)
    res = r.results()
    if d.rank == 0:
        print(json.dumps({'ranks': d.world, 'updates': len(res['pc_max']),
                          'frames': len(res['template_index']), 'templates': res['templates'],
                          'seconds': dt, 'pc_max': res['pc_max'].tolist(),
                          'template_index': res['template_index'].tolist(),
                          'em_points': res['em_points'].tolist(),
                          **({'view_offset': res['view_offset'].tolist()} if args.view_shift else {}),
                          **({'pc_pose': res['pc_pose'].tolist()} if args.subcell_peak else {}),
                          **({'experiences': r.em.poses().tolist(),
                              'links': [list(map(float, l)) for l in r.em.links().tolist()]}
                             if em is not None else {})}))
    d.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
