"""placeholder package (opencv_from_cameras_projection is fused into the GGS kernels' pose decode, csrc/pd_ggs_dev.h)"""
