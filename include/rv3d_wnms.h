/* rv3d_wnms.h -- the weighted-NMS entries that take the RV_WNMS_* choices per call.  Part of rv3d.h, which includes this file next to
 * the weighted-NMS block and documents the four choices there (the axes along which a third-party `wnms_gpu` may differ from the
 * declared semantics); not meant to be included on its own: the types, the flag values and the `extern "C"` are rv3d.h's. */
#ifndef RV3D_WNMS_H_
#define RV3D_WNMS_H_

/* the arguments of rv_wnms_classes (cats may be NULL) and `flags` (RV_WNMS_* bits; 0 = rv_wnms_classes bit for bit; a bit outside
 * the four fails with a message in rv_last_error) */
int rv_wnms_opt(const float* boxes, const float* data, const int32_t* cats, int64_t n, int32_t d, float nms_thresh,
                float merge_thresh, float* output, int64_t* keep, int64_t* count, void* workspace, int64_t* host_num_out,
                rvStream stream, int32_t flags);
/* the arguments of rv_nms_sweeps and `flags`: same workspaces, same `resume` / `out_counts` protocol, same launches */
int rv_nms_sweeps_opt(const float* scores, const int64_t* cats, const float* cuboids, int32_t B, int64_t K, int32_t n_classes,
                      float min_confidence, float nms_thresh, float merge_thresh, int32_t num_pre_nms, int32_t num_post_nms,
                      int32_t cap, int32_t out_cap, float* out_boxes, float* out_scores, int32_t* out_cats, int64_t* out_counts,
                      void* workspace, void* mask_workspace, int64_t mask_words, int32_t resume, rvStream stream, int32_t flags);

#endif /* RV3D_WNMS_H_ */
