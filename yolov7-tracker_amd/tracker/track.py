"""`tracker/track.py` of the reference (/root/reference/tracker/track.py:53-386) with the same flags, config-file
format and result-file format, driving the MI355X hot path: detector forward + decode/NMS (liby7t.so) and the
device-resident SORT / ByteTrack trackers.

    python tracker/track.py --dataset visdrone --tracker bytetrack --model_path weights/best.pt
    python tracker/track.py --dataset synthetic --tracker bytetrack --model_path random:yolov7-w6 --synthetic_dets

Extra flags (defaults reproduce the reference's behaviour): --model_cfg (yaml / arch name for state-dict checkpoints),
--nc, --synthetic_dets, --synthetic_frames/--synthetic_objs/--synthetic_seqs, --results_root, --device_preprocess, --batch,
--gmc {none,ecc,features} / --gmc_faithful 0|1 (the camera-motion estimate of tracker/gmc.py for strongsort and botsort; default none).
--augment (the detector's three-pass test-time augmentation, as detect.py --augment; default off).
--reid_half (an OSNet --reid_model_path through the general fp16 / MFMA op list: any width, the IBN variant, any crop size; default off).
--botsort_reid (with --tracker botsort: its appearance branch, use_apperance_model, with --reid_model_path features; default off, as in the reference).
--save_images / --save_videos (the reference's flags): the overlay and the JPEG encoding run on the device (tracker/render.py); the video is a Motion-JPEG AVI of the
very same JPEG files, not the reference's mp4v.
--device_decode (implies --device_preprocess): the loader hands over the JPEG files' bytes and the frames are decoded on the device (tracker/jpeg_decode.py); files
the device decoder does not take (progressive, CMYK, PNG, ...) are decoded on the host as before, and a line per sequence says how many went each way.
"""
import argparse
import os
from time import gmtime, strftime

import numpy as np
import torch
import yaml

from . import tracker_dataloader
from .basetrack import BaseTracker
from .bytetrack import ByteTrack
from .botsort import BoTSORT
from .deepsort import DeepSORT
from .c_biou_tracker import C_BIoUTracker
from .uavmot import UAVMOT
from .strongsort import StrongSORT
from .deepmot import DeepMOT
from .timer import Timer
from ..detector import attempt_load, check_img_size, non_max_suppression, scale_coords

TRACKER_DICT = {'sort': BaseTracker, 'bytetrack': ByteTrack, 'botsort': BoTSORT, 'deepsort': DeepSORT,
                'c_biou': C_BIoUTracker, 'uavmot': UAVMOT, 'strongsort': StrongSORT, 'deepmot': DeepMOT}   # track.py:56-65: all eight keys

timer = Timer()
seq_fps = []
decode_counts = {}      # --device_decode: sequence -> {'device': frames decoded on the device, 'host': frames that fell back to the host}


def post_process_v7(out, img_size, ori_img_size, conf_thres=0.01, all_images=False, classes=None, agnostic=False):
    """track.py:234-244 (the reference keeps image 0 of the batch; all_images=True returns the list for every image).
    classes / agnostic (extension): non_max_suppression's arguments of the same names, as detect.py:79 passes --classes / --agnostic-nms"""
    res = non_max_suppression(out, conf_thres=conf_thres, classes=classes, agnostic=agnostic)
    for o in res:
        o[:, :4] = scale_coords(img_size, o[:, :4], ori_img_size, ratio_pad=None).round()
    return res if all_images else res[0]


def save_results(results_root, folder_name, seq_name, results, data_type='mot17'):
    """track.py:247-273: `frame,id,x,y,w,h,1.0,-1,-1,-1` with %.2f"""
    assert len(results)
    os.makedirs(os.path.join(results_root, folder_name), exist_ok=True)
    with open(os.path.join(results_root, folder_name, seq_name + '.txt'), 'w') as f:
        for frame_id, target_ids, tlwhs, clses in results:
            for id, tlwh, cls in zip(target_ids, tlwhs, clses):
                if data_type == 'default':
                    f.write(f'{frame_id},{id},{tlwh[0]:.2f},{tlwh[1]:.2f},{tlwh[2]:.2f},{tlwh[3]:.2f},{int(cls)}\n')
                else:
                    f.write(f'{frame_id},{id},{tlwh[0]:.2f},{tlwh[1]:.2f},{tlwh[2]:.2f},{tlwh[3]:.2f},1.0,-1,-1,-1\n')
    return folder_name


def sequence_list(opts, cfgs):
    """track.py:93-109: the sequences to track -> (sorted names, folder that holds them or None).  'origin': the sub-folders of the dataset's sequence folder;
    'yolo': the parent-folder names of the image paths listed in ./<dataset>/test.txt.  IGNORE_SEQS / CERTAIN_SEQS of the dataset yaml apply to both."""
    DATASET_ROOT, CERTAIN_SEQS, IGNORE_SEQS = cfgs['DATASET_ROOT'], cfgs['CERTAIN_SEQS'], cfgs['IGNORE_SEQS']
    if opts.data_format == 'yolo':
        DATA_ROOT = None
        seqs = []
        with open(os.path.join(getattr(opts, 'yolo_root', './'), opts.dataset, 'test.txt'), 'r') as f:
            for line in f.readlines():
                elems = line.split('/')      # the sequence name is elems[-2]
                if len(elems) >= 2 and elems[-2] not in seqs:
                    seqs.append(elems[-2])
    elif opts.data_format == 'origin':
        DATA_ROOT = os.path.join(DATASET_ROOT, cfgs.get('SEQ_SUBDIR', 'VisDrone2019-MOT-test-dev/sequences'))
        seqs = os.listdir(DATA_ROOT)
    else:
        raise NotImplementedError
    seqs = sorted(seqs)
    seqs = [s for s in seqs if s not in IGNORE_SEQS]
    if None not in CERTAIN_SEQS:
        seqs = CERTAIN_SEQS
    return seqs, DATA_ROOT


def main(opts, cfgs):
    DATASET_ROOT, CERTAIN_SEQS, IGNORE_SEQS = cfgs['DATASET_ROOT'], cfgs['CERTAIN_SEQS'], cfgs['IGNORE_SEQS']
    if opts.tracker not in TRACKER_DICT:
        raise NotImplementedError("tracker %r: only %s run on the device path" % (opts.tracker, sorted(TRACKER_DICT)))
    if opts.tracker == 'botsort':
        opts.kalman_format = 'botsort'      # track.py:68-69
    elif opts.tracker == 'strongsort':
        opts.kalman_format = 'strongsort'   # track.py:70-71
    botsort_reid = bool(getattr(opts, 'botsort_reid', False))
    if botsort_reid and opts.tracker != 'botsort':
        raise ValueError("--botsort_reid: the appearance branch belongs to --tracker botsort (tracker %r has none to switch)" % (opts.tracker,))
    if opts.gmc != 'none' and opts.tracker not in ('strongsort', 'botsort'):
        raise ValueError("--gmc %s: only strongsort and botsort compensate camera motion (tracker %r does not)" % (opts.gmc, opts.tracker))
    aflink_weights = None
    if getattr(opts, 'aflink', None):
        from .aflink import load_aflink_weights
        aflink_weights = load_aflink_weights(opts.aflink)
    device_decode = bool(getattr(opts, 'device_decode', False))
    if device_decode:
        if opts.dataset == 'synthetic':
            raise ValueError("--device_decode decodes the files of a dataset: the synthetic sequences have none")
        opts.device_preprocess = True      # the decoded frame is on the device already
    img_size = opts.img_size[0] if isinstance(opts.img_size, (list, tuple)) else opts.img_size
    model = attempt_load(opts.model_path, cfg=opts.model_cfg, nc=opts.nc, img_size=img_size, max_batch=max(1, opts.batch))
    stride = int(model.stride.max())
    opts.img_size = check_img_size(img_size, s=stride)
    synthetic = opts.dataset == 'synthetic'
    if synthetic:
        seqs = ['synthetic-%03d' % i for i in range(opts.synthetic_seqs)]
    else:
        seqs, DATA_ROOT = sequence_list(opts, cfgs)
    print(f'Seqs will be evalueated, total{len(seqs)}:')
    print(seqs)
    folder_name = strftime("%Y-%d-%m %H:%M:%S", gmtime())[5:-3].replace('-', '_').replace(' ', '_').replace(':', '_')
    folder_name = opts.tracker + '_' + folder_name
    for si, seq in enumerate(seqs):
        print(f'--------------tracking seq {seq}--------------')
        if synthetic:
            loader = tracker_dataloader.SyntheticLoader(opts.synthetic_frames, opts.synthetic_objs, opts.img_size, si,
                                                        device_preprocess=opts.device_preprocess, moving_camera='corners' if opts.gmc == 'features' else opts.gmc != 'none',
                                                        miss=getattr(opts, 'synthetic_miss', None))
        else:
            # track.py:126: the sequence folder ('origin') or the path file every sequence is filtered out of ('yolo')
            path = os.path.join(DATA_ROOT, seq) if opts.data_format == 'origin' else os.path.join(getattr(opts, 'yolo_root', './'), opts.dataset, 'test.txt')
            loader = tracker_dataloader.TrackerLoader(path, opts.img_size, opts.data_format, seq,
                                                      pre_process_method='v7', model_stride=stride,
                                                      device_preprocess=opts.device_preprocess,
                                                      yolo_data_root=cfgs.get('YOLO_DATA_ROOT', DATASET_ROOT), device_decode=device_decode)
        data_loader = torch.utils.data.DataLoader(loader, batch_size=max(1, opts.batch), **({'collate_fn': tracker_dataloader.collate_bytes} if device_decode else {}))
        decoded = {'device': 0, 'host': 0}
        # (extension) --botsort_reid: BoTSORT's use_apperance_model, which the reference hard-codes to False (botsort.py:276)
        tracker = TRACKER_DICT[opts.tracker](opts, frame_rate=30, gamma=opts.gamma, **({'use_apperance_model': True} if botsort_reid else {}))
        if opts.gmc in ('ecc', 'features'):      # (extension) estimate the camera motion on the device; one estimator per sequence, like the reference's per-tracker GMC
            from .gmc import GMC
            estimator = GMC(opts.gmc, faithful=bool(opts.gmc_faithful))
            if opts.tracker == 'strongsort':
                tracker.ECC = estimator
            else:
                tracker.gmc = estimator.apply_device
        results, frame_id, i = [], 0, -1
        if opts.save_images:      # track.py:176-177: <DATASET_ROOT>/result_images/<seq>/; the synthetic dataset has no root of its own and writes beside its results
            image_dir = os.path.join(os.path.join(opts.results_root, folder_name) if synthetic else DATASET_ROOT, 'result_images', seq)
            jpeg_files = []
        for imgs, imgs0 in data_loader:
            # --batch N (extension, default 1 = the reference's frame-at-a-time loop): the detector + decode/NMS run once over N
            # consecutive frames (that is where the throughput of bench.py comes from), the tracker then takes them in order
            if device_decode:      # imgs0 is the list of the files' bytes: the frames come into being on the device (outside the timed region, like the loader's decode)
                from . import jpeg_decode
                imgs0 = jpeg_decode.decode_batch(imgs0, max_batch=max(1, opts.batch), counts=decoded)
            nb = imgs0.shape[0]
            timer.tic()
            detect = [not (i + 1 + k) % opts.detect_per_frame for k in range(nb)]
            outs = None
            if any(detect):
                # conf_thres 0.01 (track.py:239) is known here, so the Detect convs decode + filter in their epilogue (fused forward)
                if getattr(opts, 'augment', False):      # (extension) the three-pass forward of detect.py --augment: plain heads, one NMS over the union
                    if opts.device_preprocess:      # frames of the network's size only: pass 0 from the raw frame (fused stem), the scaled passes resample the same frame
                        head, lb_size = model.forward_frames_augment(imgs0, img_size=opts.img_size, conf_thres=0.01)
                    else:
                        head, lb_size = model.forward_augment(imgs.cuda(), conf_thres=0.01), imgs.shape[2:]
                elif opts.device_preprocess:      # raw uint8 frames -> letterbox + layout on the GPU
                    head, lb_size = model.forward_frames(imgs0, img_size=opts.img_size, fuse_decode=0.01)
                else:
                    head, lb_size = model.forward(imgs.cuda(), fuse_decode=0.01), imgs.shape[2:]
                outs = post_process_v7(head, img_size=lb_size, ori_img_size=imgs0.shape[1:], all_images=True, classes=opts.classes, agnostic=opts.agnostic_nms)
            for k in range(nb):
                if k:
                    timer.tic()
                i += 1
                img0 = imgs0[k]
                if detect[k]:
                    out = outs[k]
                    if opts.synthetic_dets and synthetic:
                        out = torch.from_numpy(loader.dets[i])      # the scene's detections stand in for a trained detector
                    current_tracks = tracker.update(out, img0)
                else:
                    current_tracks = tracker.update_without_detection(None, img0)
                cur_tlwh, cur_id, cur_cls = [], [], []
                for trk in current_tracks:
                    bbox = trk.tlwh
                    if bbox[2] * bbox[3] > opts.min_area:
                        cur_tlwh.append(bbox)
                        cur_id.append(trk.track_id)
                        cur_cls.append(trk.cls)
                results.append((frame_id + 1, cur_id, cur_tlwh, cur_cls))
                timer.toc()
                frame_id += 1
            if opts.save_images:      # outside the timed region, like plot_img: the batch's frames (uploaded once if they came on the host) with the rows just recorded
                from . import render
                renderer = _renderer_for(imgs0.shape[1], imgs0.shape[2], max(1, opts.batch))
                rows = [render.tracks_from_results(ids, tlwhs, clses, cfgs.get('CATEGORY_DICT')) for _, ids, tlwhs, clses in results[-nb:]]
                jpeg_files += renderer.save(imgs0, rows, [os.path.join(image_dir, f'{fid - 1:05d}.jpg') for fid, _, _, _ in results[-nb:]])
        if device_decode:
            decode_counts[seq] = decoded
            print(f"device_decode: {decoded['device']} frames decoded on the device, {decoded['host']} on the host (fallback)")
        seq_fps.append(i / timer.total_time)   # track.py:181 (sic: last index, not the frame count)
        timer.clear()
        if aflink_weights is not None:      # (extension) --aflink: the rows that would have been written, linked; the file and TrackEval see the linked ids
            from . import aflink
            results = aflink.link_results(aflink_weights, results, max_pairs=opts.aflink_max_pairs)
        if getattr(opts, 'gsi', False):      # (extension) --gsi: after --aflink (StrongSORT++'s order): short gaps filled, every track smoothed, before the file is written
            from . import gsi
            results = gsi.smooth_results(results, interval=opts.gsi_interval, tau=opts.gsi_tau)
        save_results(opts.results_root, folder_name, seq, results)
        if opts.save_images and opts.save_videos and jpeg_files:      # track.py:190-191; the chunks are the .jpg files' bytes, nothing is encoded again
            from . import render
            render.write_mjpeg_avi(os.path.join(os.path.dirname(image_dir), seq + '.avi'), jpeg_files, (imgs0.shape[2], imgs0.shape[1]), fps=15)
    print(f'average fps: {np.mean(seq_fps)}')
    if opts.track_eval and (synthetic or cfgs.get('TRACK_EVAL')):
        evaluate_results(opts, cfgs, seqs, folder_name, synthetic)
    return os.path.join(opts.results_root, folder_name)


_renderers = {}


def _renderer_for(H, W, batch):
    """one DeviceRenderer per frame size (a sequence's frames share one); its encoder takes at most 8 frames at a time, longer batches go in parts"""
    key = (int(H), int(W), min(int(batch), 8))
    if key not in _renderers:
        from .render import DeviceRenderer
        _renderers.clear()      # (the encoder's row slots are sized for the worst case: keep one size alive)
        _renderers[key] = DeviceRenderer(key[0], key[1], max_batch=key[2])
    return _renderers[key]


def evaluate_results(opts, cfgs, seqs, folder_name, synthetic):
    """track.py:196-227: HOTA / CLEAR / Identity of the result files just written, through the TrackEval-style harness
    (tracker/trackeval).  Real datasets take their `TRACK_EVAL` block from the dataset yaml like the reference; the synthetic
    dataset writes its ground truth (synth.make_ground_truth) next to the results first."""
    from . import trackeval
    eval_config = trackeval.Evaluator.get_default_eval_config()
    if synthetic:
        from .. import synth
        gt_folder = os.path.join(opts.results_root, folder_name + '_gt')
        os.makedirs(gt_folder, exist_ok=True)
        for si, seq in enumerate(seqs):
            synth.write_mot_gt(os.path.join(gt_folder, seq + '.txt'),
                               synth.make_ground_truth(opts.synthetic_frames, opts.synthetic_objs, opts.img_size, si))
        yaml_cfg = {'GT_FOLDER': gt_folder, 'TRACKERS_FOLDER': opts.results_root, 'TRACKERS_TO_EVAL': [folder_name], 'SKIP_SPLIT_FOL': True,
                    'TRACKER_SUB_FOLDER': '', 'SEQ_INFO': {seq: opts.synthetic_frames for seq in seqs}, 'GT_LOC_FORMAT': '{gt_folder}/{seq}.txt'}
        dataset_cls = trackeval.datasets.MotChallenge2DBox
    else:
        yaml_cfg = dict(cfgs['TRACK_EVAL'])
        yaml_cfg['SEQ_INFO'] = {k: v for k, v in yaml_cfg['SEQ_INFO'].items() if k in seqs}      # track.py:203-207
        assert len(yaml_cfg['SEQ_INFO']) == len(seqs)
        yaml_cfg.setdefault('TRACKERS_TO_EVAL', [folder_name])
        dataset_cls = trackeval.datasets.MotChallenge2DBox if opts.dataset in ['mot', 'uavdt'] else trackeval.datasets.VisDrone2DBox
    dataset_config = dataset_cls.get_default_dataset_config()
    dataset_config.update({k: v for k, v in yaml_cfg.items() if k in dataset_config})
    eval_config.update({k: v for k, v in yaml_cfg.items() if k in eval_config})
    metrics_config = {'METRICS': ['HOTA', 'CLEAR', 'Identity'], 'THRESHOLD': 0.5}
    metrics_list = [m(metrics_config) for m in (trackeval.metrics.HOTA, trackeval.metrics.CLEAR, trackeval.metrics.Identity)
                    if m.get_name() in metrics_config['METRICS']]
    return trackeval.Evaluator(eval_config).evaluate([dataset_cls(dataset_config)], metrics_list)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--dataset', type=str, default='visdrone', help='visdrone, or mot')
    parser.add_argument('--data_format', type=str, default='origin', help='format of reading dataset')
    parser.add_argument('--det_output_format', type=str, default='yolo', help='data format of output of detector, yolo or other')
    parser.add_argument('--tracker', type=str, default='sort', help='sort, deepsort, etc')
    parser.add_argument('--model_path', type=str, default='./weights/best.pt', help='model path')
    parser.add_argument('--trace', type=bool, default=False, help='traced model of YOLO v7')
    parser.add_argument('--img_size', nargs='+', type=int, default=1280, help='[train, test] image sizes')
    parser.add_argument('--reid_model_path', type=str, default='./weights/ckpt.t7',
                        help='path for reid model path (an OSNet or a DeepSORT net_dict checkpoint; random[:osnet|:deepsort] = seeded random weights)')
    parser.add_argument('--dhn_path', type=str, default='./weights/DHN.pth', help='path of DHN path for DeepMOT')
    parser.add_argument('--conf_thresh', type=float, default=0.2, help='filter tracks')
    parser.add_argument('--nms_thresh', type=float, default=0.7, help='thresh for NMS')
    parser.add_argument('--iou_thresh', type=float, default=0.5, help='IOU thresh to filter tracks')
    parser.add_argument('--track_buffer', type=int, default=30, help='tracking buffer')
    parser.add_argument('--gamma', type=float, default=0.1, help='param to control fusing motion and apperance dist')
    parser.add_argument('--kalman_format', type=str, default='default', help='use what kind of Kalman, default, naive, strongsort or bot-sort like')
    parser.add_argument('--batch', type=int, default=1, help='(extension) frames per detector forward; the tracker still steps frame by frame')
    parser.add_argument('--device_preprocess', action='store_true', help='(extension) letterbox raw frames on the GPU instead of in the loader')
    parser.add_argument('--device_decode', action='store_true',
                        help='(extension) decode the JPEG frames on the GPU from the files\' bytes (implies --device_preprocess); files the device decoder does not '
                             'take are decoded on the host as before')
    parser.add_argument('--gmc', type=str, default='none', choices=['none', 'ecc', 'features'],
                        help='(extension) camera-motion estimate for strongsort / botsort on the device (tracker/gmc.py): ecc = findTransformECC, '
                             'features = FAST corners, rotated BRIEF, Hamming matching and RANSAC (the applyFeaures path the reference runs as orb)')
    parser.add_argument('--reid_half', action='store_true',
                        help="(extension) run an OSNet --reid_model_path (a checkpoint or random:osnet) through the general fp16 / MFMA op list: any width, "
                             "osnet_ibn_x1_0, any crop size (default off: the fused kernel for x0_25 at 128 x 64, the fp32 op list elsewhere)")
    parser.add_argument('--botsort_reid', action='store_true',
                        help="(extension) --tracker botsort with its appearance branch (use_apperance_model, off in the reference): IoU-gated cosine fusion with "
                             "--reid_model_path features")
    parser.add_argument('--gmc_faithful', type=int, default=1, choices=[0, 1],
                        help="(extension) 1 = the reference's applyEcc as written (every frame aligned to frame 0, half-resolution translation); "
                             "0 = previous-frame template, full-resolution translation")
    parser.add_argument('--min_area', type=float, default=150, help='use to filter small bboxs')
    parser.add_argument('--save_images', action='store_true',
                        help="save tracking results (image): <frame_id:05d>.jpg under <DATASET_ROOT>/result_images/<seq>/ (--dataset synthetic: under "
                             "<results_root>/<folder>/result_images/<seq>/); drawn and JPEG-encoded on the device with this project's outline rule and bitmap font")
    parser.add_argument('--save_videos', action='store_true',
                        help="save tracking results (video), together with --save_images: <seq>.avi beside the image folder, a Motion-JPEG AVI at 15 fps made of the "
                             "same JPEG files -- NOT the reference's mp4v container, which needs a codec library")
    parser.add_argument('--detect_per_frame', type=int, default=1, help='choose how many frames per detect')
    parser.add_argument('--track_eval', type=bool, default=True, help='Use TrackEval to evaluate')
    # additions (defaults keep the reference's behaviour)
    parser.add_argument('--model_cfg', type=str, default=None, help='model yaml / arch name for state-dict checkpoints')
    parser.add_argument('--nc', type=int, default=None)
    parser.add_argument('--synthetic_dets', action='store_true', help='--dataset synthetic: feed the scene detections to the tracker')
    parser.add_argument('--synthetic_frames', type=int, default=100)
    parser.add_argument('--synthetic_objs', type=int, default=80)
    parser.add_argument('--synthetic_seqs', type=int, default=1)
    parser.add_argument('--synthetic_miss', type=float, default=None, help="--dataset synthetic: the scene detections' miss rate (default: the generator's 0.10)")
    parser.add_argument('--results_root', type=str, default='./tracker/results')
    parser.add_argument('--aflink', type=str, default=None,
                        help="(extension) link fragmented tracklets after each sequence with AFLink (tracker/aflink.py): a PostLinker state dict file, or "
                             "random:aflink[:seed[:gain]]; default off")
    parser.add_argument('--aflink_max_pairs', type=int, default=65536, help='(extension) --aflink: capacity of the candidate pair list')
    parser.add_argument('--gsi', action='store_true',
                        help="(extension) after each sequence (and after --aflink), fill the gaps shorter than --gsi_interval frames linearly and smooth every track with "
                             "GSI (tracker/gsi.py); the rows GSI adds are not filtered by --min_area again; default off")
    parser.add_argument('--gsi_interval', type=int, default=20, help='(extension) --gsi: gaps of fewer than this many frames are filled')
    parser.add_argument('--gsi_tau', type=float, default=10, help="(extension) --gsi: the smoother's time constant")
    parser.add_argument('--yolo_root', type=str, default='./', help="(extension) where ./<dataset>/test.txt of --data_format yolo lives (the reference: the working directory)")
    # the NMS arguments of the reference's detect.py:166-167 (non_max_suppression applies them before its max_nms / max_det cuts)
    parser.add_argument('--classes', nargs='+', type=int, default=None, help='(extension) filter by class: --classes 0, or --classes 0 2 3')
    parser.add_argument('--agnostic_nms', action='store_true', help='(extension) class-agnostic NMS')
    parser.add_argument('--augment', action='store_true',
                        help="(extension) augmented inference, detect.py / test.py --augment of the reference (models/yolo.py:301-317): three passes at scales 1, 0.83, 0.67, the "
                             "middle one flipped left-right, one NMS over their union; with --device_preprocess only for frames of the network's size (no letterboxing)")
    return parser


def cli(argv=None):
    opts = build_parser().parse_args(argv)
    if opts.dataset == 'synthetic':
        cfgs = {'DATASET_ROOT': '', 'CERTAIN_SEQS': [None], 'IGNORE_SEQS': [None], 'CATEGORY_DICT': {}, 'YAML_DICT': ''}
    else:
        path = f'./tracker/config_files/{opts.dataset}.yaml'
        if not os.path.isfile(path):
            path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'config_files', f'{opts.dataset}.yaml')
        with open(path, 'r') as f:
            cfgs = yaml.load(f, Loader=yaml.FullLoader)
    return main(opts, cfgs)


if __name__ == '__main__':
    cli()
