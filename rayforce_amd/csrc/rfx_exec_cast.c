/* rfx_exec_cast.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * `as` over vectors (rfx_cast.hip): an element-wise map, so it runs over every shard's rows (rfx_exec_split) like the bucket verbs' maps: each shard
 * casts its row range into its own piece of the result, no shard reads another's cells. */
int rfx_exec_cast(rfx_exec_t *x, int32_t src_type, int32_t dst_type, const void *const *d_ins, int64_t n, void *const *d_outs, int shard) {
    if (!x || !d_ins || !d_outs || n < 0 || shard >= x->nshards) return RFX_EINVAL;
    x->err[0] = 0;
    if (x->has_tr) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: cast over several ranks");
        return RFX_ELIMIT;
    }
    if (!rfx_hip_cast_arm(src_type, dst_type)) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: cast: the reference has no cast from type %d to type %d", (int)(src_type & ~RFX_CAST_WIDENED), (int)dst_type);
        return RFX_EINVAL;
    }
    int rc = RFX_OK;
    if (shard >= 0) rc = rfx_hip_cast(x->ctx[shard], src_type, dst_type, d_ins[shard], n, d_outs[shard]);
    else {
        for (int s = 0; s < x->nshards && rc == RFX_OK; s++) {
            int64_t r0, len;
            rfx_exec_split(n, x->nshards, s, &r0, &len);
            if (len <= 0) continue;
            if (x->nshards > 1) rfx_hip_ctx_bind_thread(x->ctx[s]);
            rc = rfx_hip_cast(x->ctx[s], src_type, dst_type, d_ins[s], len, d_outs[s]);
        }
        if (x->nshards > 1) {
            for (int s = 0; s < x->nshards; s++) { /* everything enqueued, then one wait per shard */
                rfx_hip_ctx_bind_thread(x->ctx[s]);
                const int src = rfx_hip_ctx_sync(x->ctx[s]);
                if (rc == RFX_OK) rc = src;
            }
            rfx_hip_ctx_bind_thread(x->ctx[0]);
        }
    }
    if (rc == RFX_OK) x->stat[RFX_XSTAT_CASTS]++;
    else snprintf(x->err, sizeof(x->err), "rfx_exec: cast: %s", rfx_hip_last_error());
    return rc;
}
