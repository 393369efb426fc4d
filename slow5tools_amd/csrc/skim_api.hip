// skim_api.hip — slow5tools skim (src/skim.c) for a whole chunk of BLOW5 records: the header's layout, then
// upload -> inflate (zlib / zstd; record press none is read where it lies) -> k_skim_format measure -> scan -> k_skim_format write
// -> one D2H of finished text.  Only compressed bytes go up and only the lines come back.
#include <string>

#include "host_ctx.h"
#include "skim_dev.h"

namespace {

bool name_is(const char *p, size_t n, const char *lit) { return strlen(lit) == n && memcmp(p, lit, n) == 0; }

// the role skim gives a field by its name (src/skim.c:227-260), and the type slow5lib's getter for that role insists on
struct RoleRule { const char *name; uint8_t role; uint8_t type; };
const RoleRule kRoles[] = {
    {"channel_number", S5GPU_SKIM_STRING, S5GPU_AUX_CHAR | S5GPU_AUX_ARRAY},
    {"median_before", S5GPU_SKIM_DOUBLE, S5GPU_AUX_DOUBLE},
    {"read_number", S5GPU_SKIM_INT32, S5GPU_AUX_INT32},
    {"start_mux", S5GPU_SKIM_UINT8, S5GPU_AUX_UINT8},
    {"start_time", S5GPU_SKIM_UINT64, S5GPU_AUX_UINT64},
    {"end_reason", S5GPU_SKIM_ENUM, S5GPU_AUX_ENUM},
    {"tracked_scaling_shift", S5GPU_SKIM_FLOAT, S5GPU_AUX_FLOAT},
    {"tracked_scaling_scale", S5GPU_SKIM_FLOAT, S5GPU_AUX_FLOAT},
    {"predicted_scaling_shift", S5GPU_SKIM_FLOAT, S5GPU_AUX_FLOAT},
    {"predicted_scaling_scale", S5GPU_SKIM_FLOAT, S5GPU_AUX_FLOAT},
    {"num_reads_since_mux_change", S5GPU_SKIM_UINT32, S5GPU_AUX_UINT32},
    {"time_since_mux_change", S5GPU_SKIM_FLOAT, S5GPU_AUX_FLOAT},
    {"num_minknow_events", S5GPU_SKIM_UINT64, S5GPU_AUX_UINT64},
};

// the tab-separated columns of one header line (without its leading '#')
std::vector<std::pair<const char *, size_t>> columns(const char *p, size_t n) {
    std::vector<std::pair<const char *, size_t>> c;
    size_t b = 0;
    while (b <= n) {
        const char *t = (const char *)memchr(p + b, '\t', n - b);
        const size_t l = t ? (size_t)(t - p) - b : n - b;
        c.emplace_back(p + b, l);
        b += l + 1;
    }
    return c;
}

// the line of the header text that starts with `lead` (without the newline), or false
bool find_line(const char *h, size_t len, const char *lead, const char **line, size_t *n) {
    const size_t ll = strlen(lead);
    size_t b = 0;
    while (b < len) {
        const char *e = (const char *)memchr(h + b, '\n', len - b);
        size_t l = e ? (size_t)(e - h) - b : len - b;
        if (l >= ll && memcmp(h + b, lead, ll) == 0) {
            while (l && h[b + l - 1] == '\r') l--;
            *line = h + b;
            *n = l;
            return true;
        }
        b += l + 1;
    }
    return false;
}

}  // namespace

extern "C" int s5gpu_skim_layout_parse(const char *header, size_t len, s5gpu_skim_layout_t *L) {
    if (!header || !L) { s5gpu_set_error("s5gpu_skim_layout_parse: NULL argument"); return S5GPU_ERR_ARG; }
    memset(L, 0, sizeof *L);
    const char *tl, *nl;
    size_t tn, nn;
    if (!find_line(header, len, "#char*", &tl, &tn) || !find_line(header, len, "#read_id", &nl, &nn)) {
        s5gpu_set_error("s5gpu_skim_layout_parse: the header has no column types line or no column names line");
        return S5GPU_ERR_DATA;
    }
    uint8_t types[S5GPU_SKIM_MAX_AUX];
    const int k = s5gpu_aux_types_parse(tl, tn, types, S5GPU_SKIM_MAX_AUX);
    if (k < 0) return k;
    const auto tcol = columns(tl + 1, tn - 1), ncol = columns(nl + 1, nn - 1);
    if (ncol.size() != tcol.size() || ncol.size() != 8u + (size_t)k) {
        s5gpu_set_error("s5gpu_skim_layout_parse: %zu column names for %zu column types", ncol.size(), tcol.size());
        return S5GPU_ERR_DATA;
    }
    L->n_aux = (uint32_t)k;
    uint32_t at = 0, nlab = 0;
    auto keep = [&](const char *p, size_t n, uint32_t *off) -> bool {
        if (at + n > S5GPU_SKIM_TEXT) return false;
        memcpy(L->text + at, p, n);
        *off = at;
        at += (uint32_t)n;
        return true;
    };
    for (int a = 0; a < k; a++) {
        const char *nm = ncol[8 + a].first;
        const size_t nlen = ncol[8 + a].second;
        L->type[a] = types[a];
        L->name_len[a] = (uint32_t)nlen;
        if (!keep(nm, nlen, &L->name_off[a])) { s5gpu_set_error("s5gpu_skim_layout_parse: more than %d bytes of names and labels", S5GPU_SKIM_TEXT); return S5GPU_ERR_ARG; }
        L->role[a] = S5GPU_SKIM_DOT;
        for (const RoleRule &r : kRoles) {
            if (!name_is(nm, nlen, r.name)) continue;
            if (types[a] != r.type) {
                s5gpu_set_error("aux field '%s' is declared '%.*s', which skim cannot read as its own type", r.name, (int)tcol[8 + a].second, tcol[8 + a].first);
                return S5GPU_ERR_DATA;
            }
            L->role[a] = r.role;
        }
        if (L->role[a] == S5GPU_SKIM_DOT) L->n_unhandled++;
        if (L->role[a] == S5GPU_SKIM_ENUM) {          // "enum{a,b,c}": the labels
            const char *p = tcol[8 + a].first + 5;
            const size_t n = tcol[8 + a].second - 6;
            L->label_first[a] = (uint16_t)nlab;
            size_t b = 0;
            while (b <= n) {
                const char *c = (const char *)memchr(p + b, ',', n - b);
                const size_t l = c ? (size_t)(c - p) - b : n - b;
                if (nlab >= S5GPU_SKIM_MAX_LABELS || L->n_labels[a] >= 255 || l > 0xFFFF) {
                    s5gpu_set_error("s5gpu_skim_layout_parse: too many enum labels");
                    return S5GPU_ERR_ARG;
                }
                if (!keep(p + b, l, &L->label_off[nlab])) { s5gpu_set_error("s5gpu_skim_layout_parse: more than %d bytes of names and labels", S5GPU_SKIM_TEXT); return S5GPU_ERR_ARG; }
                L->label_len[nlab++] = (uint16_t)l;
                L->n_labels[a]++;
                b += l + 1;
            }
        }
    }
    L->n_labels_total = nlab;
    L->text_len = at;
    return S5GPU_OK;
}

// One device's share of a chunk: records [lo, hi).  Returns the share's lines through sg (ShareGather) into out_buf.
static int skim_share(int slot, uint32_t lo, uint32_t hi, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                      int sig_method, const s5gpu_skim_layout_t *layout, void *out_buf, size_t out_cap, uint64_t *out_off, int32_t *status, uint32_t n,
                      s5host::ShareGather &sg) {
    s5host::CtxHold hold;
    int r = hold.acquire(slot);
    if (r) return sg.fail(r, slot);
    Ctx *c = hold.c;
    const uint32_t m = hi - lo;
    auto hip = [&](hipError_t e, const char *what) -> int {
        if (e == hipSuccess) return 0;
        s5gpu_set_error("%s failed: %s", what, hipGetErrorString(e));
        return sg.fail(S5GPU_ERR_HIP, slot);
    };
    uint64_t b0, e1;                                   // (this share's part of the span: the bounds held for the whole batch)
    (void)s5rules::chunk_span("s5gpu_skim_stream", "record", m, chunk_bytes, rec_pos + lo, rec_len + lo, &b0, &e1);
    const uint8_t *base = (const uint8_t *)chunk + b0;
    const bool packed = rec_method != S5GPU_REC_NONE;
    // device table: layout | len (u32 m) | status (i32 m) | off (u64 m + 1) | scan scratch
    const size_t o_len = up(sizeof(s5gpu_skim_layout_t), 256), o_st = o_len + up(4ull * m, 256), o_off = o_st + up(4ull * m, 256),
                 o_tmp = o_off + up(8ull * (m + 1), 256), b_all = o_tmp + 8ull * (m / 1024 + 8);
    if ((r = c->d_in.reserve(e1 - b0 + 64)) || (r = c->d_tdesc.reserve(b_all)) || (r = c->d_desc2.reserve(sizeof(s5gpu_rec_desc_t) * m)) ||
        (r = c->h_in.reserve(sizeof(s5gpu_rec_desc_t) * m + 64)) || (r = c->h_out.reserve(4ull * m + 64)))
        return sg.fail(r, slot);
    uint8_t *dv = (uint8_t *)c->d_tdesc.p;
    uint32_t *d_len = (uint32_t *)(dv + o_len);
    int32_t *d_st = (int32_t *)(dv + o_st);
    uint64_t *d_off = (uint64_t *)(dv + o_off), *d_tmp = (uint64_t *)(dv + o_tmp);
    if ((r = hip(hipMemcpyAsync(c->d_in.p, base, e1 - b0, hipMemcpyHostToDevice, c->st), "upload of the chunk"))) return r;
    if ((r = hip(hipMemcpyAsync(dv, layout, sizeof *layout, hipMemcpyHostToDevice, c->st), "upload of the layout"))) return r;
    s5_trace("skim: chunk uploaded");
    std::vector<s5gpu_rec_desc_t> rd(m);
    std::vector<uint32_t> pcap(m);
    for (uint32_t i = 0; i < m; i++) {
        const uint64_t g = packed ? s5host::payload_guess_of(rec_method, (const uint8_t *)chunk + rec_pos[lo + i], rec_len[lo + i]) : 0;
        pcap[i] = s5rules::first_cap(g);
    }
    skim::SkimArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.n = m; sa.sig_method = sig_method;
    sa.desc = (const s5gpu_rec_desc_t *)c->d_desc2.p;
    sa.plan = (const s5gpu_skim_layout_t *)dv;
    sa.len = d_len; sa.status = d_st; sa.off = d_off;
    const int32_t *hs = (const int32_t *)c->h_out.p;
    for (int attempt = 0;; attempt++) {
        uint64_t po = 0;
        uint32_t max_cap = 0;
        for (uint32_t i = 0; i < m; i++) {
            s5gpu_rec_desc_t &d = rd[i];
            memset(&d, 0, sizeof d);
            d.in_off = rec_pos[lo + i] - b0; d.in_len = rec_len[lo + i];
            d.pay_off = po; d.pay_cap = pcap[i];
            po += up((uint64_t)pcap[i] + 16, 16);
            max_cap = max_cap > pcap[i] ? max_cap : pcap[i];
        }
        memcpy(c->h_in.p, rd.data(), sizeof(s5gpu_rec_desc_t) * m);
        if ((r = hip(hipMemcpyAsync(c->d_desc2.p, c->h_in.p, sizeof(s5gpu_rec_desc_t) * m, hipMemcpyHostToDevice, c->st), "upload"))) return r;
        if (packed) {
            if ((r = c->d_pay.reserve(po + 64)) || (r = c->d_fields.reserve(sizeof(s5gpu_rec_fields_t) * m))) return sg.fail(r, slot);
            if ((r = hip(hipMemsetAsync(c->d_fields.p, 0, sizeof(s5gpu_rec_fields_t) * m, c->st), "memset"))) return r;
            s5gpu_decode_args_t da;
            memset(&da, 0, sizeof da);
            da.n_recs = m; da.rec_method = rec_method; da.sig_method = sig_method;
            da.desc = (const s5gpu_rec_desc_t *)c->d_desc2.p; da.in = (const uint8_t *)c->d_in.p;
            da.payload = (uint8_t *)c->d_pay.p; da.fields = (s5gpu_rec_fields_t *)c->d_fields.p;
            da.max_pay_cap = max_cap;
            if ((r = s5gpu_inflate_dev(&da, c->st))) return sg.fail(r, slot);
            sa.fields = (const s5gpu_rec_fields_t *)c->d_fields.p;
            sa.pay = (const uint8_t *)c->d_pay.p;
        } else {
            sa.fields = nullptr;
            sa.pay = (const uint8_t *)c->d_in.p;
        }
        if ((r = s5_skim_measure(sa, c->st))) return sg.fail(r, slot);
        if ((r = hip(hipMemcpyAsync(c->h_out.p, d_st, 4ull * m, hipMemcpyDeviceToHost, c->st), "status download"))) return r;
        if ((r = hip(hipStreamSynchronize(c->st), "synchronise"))) return r;
        s5_trace("skim: inflated and measured");
        bool retry = false, bad = false;
        for (uint32_t i = 0; i < m; i++) {
            if (hs[i] == 5 && packed && attempt < 2) {   // a record inflated to more than its guessed slot: redo with the size it needs
                s5gpu_rec_fields_t f;
                if ((r = hip(hipMemcpy(&f, (const s5gpu_rec_fields_t *)c->d_fields.p + i, sizeof f, hipMemcpyDeviceToHost), "download"))) return r;
                pcap[i] = s5rules::grown_cap(pcap[i], f.payload_len);
                retry = true;
            } else if (hs[i] > 0) {
                bad = true;
                if (status) status[lo + i] = hs[i];
            }
        }
        if (bad) { s5gpu_set_error("s5gpu_skim_stream: at least one record is corrupt (see status[i])"); return sg.fail(S5GPU_ERR_DATA, slot); }
        if (!retry) break;
    }
    // lines with a double the device does not print (|v| >= 2^107): printed here from their payloads
    std::vector<uint32_t> h_idx, h_len;
    std::vector<uint64_t> h_off;
    std::string h_text;
    for (uint32_t i = 0; i < m; i++) {
        if (hs[i] != skim::SKIM_HOST) continue;
        uint64_t plen = rec_len[lo + i], poff = 0;
        if (packed) {
            s5gpu_rec_fields_t f;
            if ((r = hip(hipMemcpy(&f, (const s5gpu_rec_fields_t *)c->d_fields.p + i, sizeof f, hipMemcpyDeviceToHost), "download"))) return r;
            plen = f.payload_len; poff = rd[i].pay_off;
        }
        std::vector<uint8_t> pay(plen + 1);
        if (packed) { if ((r = hip(hipMemcpy(pay.data(), (const uint8_t *)c->d_pay.p + poff, plen, hipMemcpyDeviceToHost), "download"))) return r; }
        else memcpy(pay.data(), (const uint8_t *)chunk + rec_pos[lo + i], plen);
        skim::Sink cnt(nullptr);
        int st = skim::skim_line(pay.data(), plen, sig_method, layout, cnt);
        if (st == 0 && cnt.n > 0xFFFFFFFFull) st = 7;
        if (st) { if (status) status[lo + i] = st; s5gpu_set_error("s5gpu_skim_stream: record %u is corrupt", lo + i); return sg.fail(S5GPU_ERR_DATA, slot); }
        const size_t at = up(h_text.size(), 8);
        h_text.resize(at + cnt.n);
        skim::Sink o((uint8_t *)&h_text[at]);
        skim::skim_line(pay.data(), plen, sig_method, layout, o);
        o.flush();
        h_idx.push_back(i); h_len.push_back((uint32_t)cnt.n); h_off.push_back(at);
    }
    const uint32_t n_host = (uint32_t)h_idx.size();
    if (n_host) {
        const size_t k4 = up(4ull * n_host, 64), k8 = up(8ull * n_host, 64), bytes = 2 * k4 + k8 + h_text.size();
        if ((r = c->d_gather.reserve(bytes + 64)) || (r = c->h_in.reserve(bytes + 64))) return sg.fail(r, slot);
        uint8_t *h = (uint8_t *)c->h_in.p, *dg = (uint8_t *)c->d_gather.p;
        memcpy(h, h_idx.data(), 4ull * n_host); memcpy(h + k4, h_len.data(), 4ull * n_host); memcpy(h + 2 * k4, h_off.data(), 8ull * n_host);
        memcpy(h + 2 * k4 + k8, h_text.data(), h_text.size());
        if ((r = hip(hipMemcpyAsync(dg, h, bytes, hipMemcpyHostToDevice, c->st), "upload of the host lines"))) return r;
        if ((r = s5_skim_patch_len(d_len, n_host, (const uint32_t *)dg, (const uint32_t *)(dg + k4), c->st))) return sg.fail(r, slot);
        sa.n_host = n_host; sa.host_idx = (const uint32_t *)dg; sa.host_off = (const uint64_t *)(dg + 2 * k4); sa.host_text = dg + 2 * k4 + k8;
    }
    if ((r = s5_scan_lengths(d_len, m, d_off, d_tmp, c->st))) return sg.fail(r, slot);
    uint64_t total = 0;
    if ((r = hip(hipMemcpyAsync(c->h_out.p, d_off + m, 8, hipMemcpyDeviceToHost, c->st), "download"))) return r;
    if ((r = hip(hipStreamSynchronize(c->st), "synchronise"))) return r;
    memcpy(&total, c->h_out.p, 8);
    s5_trace("skim: lines placed");
    uint64_t ob = 0;
    bool copy = false;
    if ((r = sg.place(slot, total, out_cap, &ob, &copy))) return r;
    if (!copy) return S5GPU_OK;
    if ((r = c->d_stream.reserve(total + 64))) return sg.fail(r, slot);
    sa.out = (uint8_t *)c->d_stream.p;
    if ((r = s5_skim_write(sa, c->st))) return sg.fail(r, slot);
    if (total && (r = hip(hipMemcpyAsync((uint8_t *)out_buf + ob, c->d_stream.p, total, hipMemcpyDeviceToHost, c->st), "text download"))) return r;
    if ((r = hip(hipMemcpyAsync(out_off + lo, d_off, 8ull * m, hipMemcpyDeviceToHost, c->st), "offset download"))) return r;
    if ((r = hip(hipStreamSynchronize(c->st), "synchronise"))) return r;
    for (uint32_t i = 0; i < m; i++) out_off[lo + i] += ob;
    if (hi == n) out_off[n] = ob + total;
    s5_trace("skim: lines downloaded");
    return S5GPU_OK;
}

extern "C" int s5gpu_skim_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                                 int sig_method, const s5gpu_skim_layout_t *layout, void *out_buf, size_t out_cap, uint64_t *out_off, int32_t *status) {
    if (n == 0) { if (out_off) out_off[0] = 0; return S5GPU_OK; }
    if (!chunk || !rec_pos || !rec_len || !layout || !out_buf || !out_off) { s5gpu_set_error("s5gpu_skim_stream: NULL argument"); return S5GPU_ERR_ARG; }
    if (!s5rules::methods_ok(rec_method, sig_method)) { s5gpu_set_error("s5gpu_skim_stream: unsupported method"); return S5GPU_ERR_ARG; }
    if (layout->n_aux > S5GPU_SKIM_MAX_AUX) { s5gpu_set_error("s5gpu_skim_stream: layout with %u aux fields", layout->n_aux); return S5GPU_ERR_ARG; }
    for (uint32_t a = 0; a < layout->n_aux; a++)
        if (layout->role[a] == S5GPU_SKIM_ENUM && (uint32_t)layout->label_first[a] + layout->n_labels[a] > S5GPU_SKIM_MAX_LABELS) {
            s5gpu_set_error("s5gpu_skim_stream: layout with labels past its table");
            return S5GPU_ERR_ARG;
        }
    // the device copy of the layout is read where its label entries point: every label of an enum field inside text[]
    for (uint32_t a = 0; a < layout->n_aux; a++) {
        if (layout->role[a] != S5GPU_SKIM_ENUM) continue;
        for (uint32_t l = layout->label_first[a], e = l + layout->n_labels[a]; l < e; l++)
            if ((uint64_t)layout->label_off[l] + layout->label_len[l] > S5GPU_SKIM_TEXT) {
                s5gpu_set_error("s5gpu_skim_stream: layout with label %u past its text", l);
                return S5GPU_ERR_ARG;
            }
    }
    if (status) memset(status, 0, sizeof(int32_t) * n);
    if (s5rules::chunk_span("s5gpu_skim_stream", "record", n, chunk_bytes, rec_pos, rec_len, nullptr, nullptr)) return S5GPU_ERR_ARG;
    const int G = s5host::n_devices();
    if (G == 0) return S5GPU_ERR_NODEV;
    s5host::ShareGather sg(G);
    const int rc = s5host::for_each_device_range(n, [&](int slot, uint32_t lo, uint32_t hi) -> int {
        const int r = skim_share(slot, lo, hi, chunk, chunk_bytes, rec_pos, rec_len, rec_method, sig_method, layout, out_buf, out_cap, out_off, status, n, sg);
        if (r) sg.fail(r, slot);
        return r;
    });
    if (rc) return sg.report(rc);   // the share that failed first, not the lowest slot that noticed
    if (sg.overflow) {
        out_off[0] = sg.need();
        s5gpu_set_error("s5gpu_skim_stream: output buffer too small (%llu bytes needed)", (unsigned long long)out_off[0]);
        return S5GPU_ERR_NOMEM;
    }
    return S5GPU_OK;
}

// the pointer-array form: the records are framed into one buffer, skimmed as a chunk, and every line handed out as a malloc'd buffer
extern "C" int s5gpu_skim_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, const s5gpu_skim_layout_t *layout,
                                void **out, size_t *out_len, int32_t *status) {
    if (n == 0) return S5GPU_OK;
    if (!rec || !rec_len || !layout || !out || !out_len) { s5gpu_set_error("s5gpu_skim_batch: NULL argument"); return S5GPU_ERR_ARG; }
    for (uint32_t i = 0; i < n; i++) { out[i] = NULL; out_len[i] = 0; }
    std::vector<uint64_t> pos(n), off(n + 1);
    std::vector<uint32_t> len(n);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (rec_len[i] > 0xFFFFFF00ull) { s5gpu_set_error("record %u too large", i); return S5GPU_ERR_ARG; }
        pos[i] = at; len[i] = (uint32_t)rec_len[i];
        at += up(rec_len[i], 16);
    }
    std::vector<uint8_t> chunk(at + 16);
    for (uint32_t i = 0; i < n; i++) if (len[i]) memcpy(chunk.data() + pos[i], rec[i], len[i]);
    std::vector<uint8_t> text(192ull * n + 4096);
    int rc = s5gpu_skim_stream(n, chunk.data(), at, pos.data(), len.data(), rec_method, sig_method, layout, text.data(), text.size(), off.data(), status);
    if (rc == S5GPU_ERR_NOMEM) {
        text.resize(off[0]);
        rc = s5gpu_skim_stream(n, chunk.data(), at, pos.data(), len.data(), rec_method, sig_method, layout, text.data(), text.size(), off.data(), status);
    }
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) {
        const size_t l = off[i + 1] - off[i];
        out[i] = malloc(l + 1);                   // + a terminating NUL: the reference's print loop takes the line as a C string
        if (!out[i]) {
            for (uint32_t j = 0; j < i; j++) { free(out[j]); out[j] = NULL; out_len[j] = 0; }
            s5gpu_set_error("s5gpu_skim_batch: out of host memory");
            return S5GPU_ERR_NOMEM;
        }
        memcpy(out[i], text.data() + off[i], l);
        ((char *)out[i])[l] = '\0';
        out_len[i] = l;
    }
    return S5GPU_OK;
}
