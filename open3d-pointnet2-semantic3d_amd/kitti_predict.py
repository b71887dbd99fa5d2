"""Labels for KITTI LiDAR frames: the reference's kitti_predict.py (PredictInterpolator), without its visualiser.

    predictor = PredictInterpolator(checkpoint_path, dataset.num_classes, model.SEMANTIC_NO_COLOR_HYPERPARAMS)
    for frame in dataset.list_file_data:                                  # dataset.KittiDataset
        dense_labels, dense_colors = predictor.label_frame(frame)         # one label per point of frame.points

Per frame: one sample of num_point points (dataset.KittiFileData.get_batch_of_one_z_box_from_origin), the colourless forward
and argmax (predict.Predictor: one captured graph per batch shape, replayed for every later frame), and the 3-NN vote of the
sparse labels onto the whole cropped frame (interpolate_label_with_color).  Nothing is captured here and no stream is made:
the Predictor is used as it is.  After the frame's construction nothing on this path waits for the device.
"""
import torch

from .cluster import _device_of, describe_clusters, euclidean_clusters
from .icp import registration_icp
from .neighbors import estimate_normals
from .plane import segment_plane
from .predict import Predictor, _on_device


class PredictInterpolator:
    """kitti_predict.py:30-104.  checkpoint_path: a file written by train.Trainer.save(), or None for fresh variables."""

    def __init__(self, checkpoint_path, num_classes, hyper_params, device="cuda"):
        self.hp = dict(hyper_params)
        self.predictor = Predictor(checkpoint_path, num_classes, self.hp, device=device)
        self.device = self.predictor.device

    def predict_and_interpolate(self, sparse_points_centered_batched, sparse_points_batched, dense_points):
        """sparse_points_centered_batched (B,N,3): the network's input; sparse_points_batched (B,N,3): the same points
        uncentred; dense_points (nd,3).  Device tensors or numpy arrays of any float dtype: they are cast to float32, as the
        reference's placeholders do (:35,57,59).  Any batch is flattened to (B*N,3) sparse points (:49,58).
        -> dense_labels (nd,) int32, dense_colors (nd,3) uint8 on the device: the majority label of the 3 nearest sparse points
        (:100) and its colour."""
        sparse_labels = self.predictor.predict(_on_device(sparse_points_centered_batched, torch.float32, self.device))
        sparse_points = _on_device(sparse_points_batched, torch.float32, self.device).reshape(-1, 3)
        return self.predictor.interpolate_labels(sparse_points, sparse_labels.reshape(-1), dense_points)

    def label_frame(self, file_data):
        """(extension) a dataset.KittiFileData -> (dense_labels, dense_colors) for file_data.points: the body of the reference's
        frame loop (:175-191)"""
        centered, raw = file_data.get_batch_of_one_z_box_from_origin(self.hp["num_point"])
        return self.predict_and_interpolate(centered, raw, file_data.points)

    def labels_for_raw_frame(self, file_data, dense_labels, n):
        """(extension) dense_labels (cnt,) of file_data.points scattered back to the n rows of the raw frame -> (n,) int32, -1
        for the rows the crop dropped"""
        out = torch.full((int(n),), -1, dtype=torch.int32, device=dense_labels.device)
        out[file_data.source_index.long()] = dense_labels.to(torch.int32)
        return out

    def objects_for_frame(self, file_data, dense_labels, eps, classes, min_points=1, max_points=None, exclude=None):
        """(extension) the labelled points of file_data.points grouped into objects: cluster.euclidean_clusters over the points
        whose dense label is one of `classes`, two points in one object when a chain of steps of at most eps joins them
        -> cluster.Clusters (ids index file_data.points).  Eager: reads the number of objects back.
        exclude: an optional (n,) bool mask of points to leave out, such as ground_for_frame(...).inliers: their label becomes -1
        before clustering."""
        if exclude is not None:
            dense_labels = _on_device(dense_labels, torch.int32, _device_of(file_data.points, dense_labels))
            exclude = _on_device(exclude, torch.bool, dense_labels.device)
            if exclude.shape != dense_labels.shape:
                raise ValueError("exclude: one bool per point")
            dense_labels = torch.where(exclude, torch.full_like(dense_labels, -1), dense_labels)
        return euclidean_clusters(file_data.points, eps, labels=dense_labels, classes=classes, min_points=min_points,
                                  max_points=max_points)

    def describe_objects(self, file_data, clusters, upright=True):
        """(extension) what each object of objects_for_frame looks like: cluster.describe_clusters over file_data.points
        -> cluster.Boxes: centroid, axes, oriented box and size per object.  upright (the default here): a vehicle stands on the
        road, so the box turns about the z axis only and Boxes.yaw() is its heading."""
        return describe_clusters(file_data.points, clusters, upright=upright)

    def normals_for_frame(self, file_data, radius, min_neighbors=3):
        """(extension) the surface normal at every point of file_data.points from the points within `radius` of it:
        neighbors.estimate_normals with the viewpoint at the sensor, (0,0,0), so every normal faces it -> (n,3) float32, NaN
        where fewer than min_neighbors points lie within the radius.  Eager."""
        return estimate_normals(file_data.points, radius, viewpoint=(0.0, 0.0, 0.0), min_neighbors=min_neighbors)

    def align_frames(self, prev_file_data, file_data, max_distance, estimation="point_to_point", init=None, normal_radius=None,
                     prev_dense_labels=None, dense_labels=None, classes=None, max_iteration=30, relative_fitness=1e-6,
                     relative_rmse=1e-6, trace=False):
        """(extension) the rigid motion that lays file_data.points (the source) onto prev_file_data.points (the target):
        icp.registration_icp.  estimation "point_to_plane" takes the target's normals from normals_for_frame(prev_file_data,
        normal_radius), normal_radius defaulting to 2 * max_distance.  classes: register on these classes of the two frames'
        dense labels only -- the static ones, so that moving objects do not drag the pose.  -> icp.RegistrationResult;
        .transformation maps this frame into the previous one's coordinates.  Eager."""
        if (classes is not None) and (prev_dense_labels is None or dense_labels is None):
            raise ValueError("classes: needs prev_dense_labels and dense_labels")
        normals = None
        if estimation == "point_to_plane":
            normals = self.normals_for_frame(prev_file_data, 2.0 * max_distance if normal_radius is None else normal_radius)
        return registration_icp(file_data.points, prev_file_data.points, max_distance, init=init, estimation=estimation,
                                target_normals=normals, max_iteration=max_iteration, relative_fitness=relative_fitness,
                                relative_rmse=relative_rmse, source_labels=dense_labels, target_labels=prev_dense_labels,
                                classes=classes, trace=trace)

    def ground_for_frame(self, file_data, distance_threshold, trials=1024, seed=0, max_angle=15.0, dense_labels=None, classes=None):
        """(extension) the ground of file_data.points: plane.segment_plane with the axis (0,0,1), the normal within max_angle
        degrees of it and pointing up, over the points whose dense label is one of `classes` (every point without dense_labels)
        -> plane.Plane; .inliers is the `exclude` of objects_for_frame, .distance(points) the height above ground.  Eager."""
        return segment_plane(file_data.points, distance_threshold, trials=trials, seed=seed, labels=dense_labels, classes=classes,
                             axis=(0.0, 0.0, 1.0), max_angle=max_angle)
