// Baseline JPEG (MJPEG) luma decode, and its colour form that keeps the chroma planes: the host half.  Parses
// each frame's markers up to SOS (never an entropy-coded byte), deduplicates the Huffman and quantisation tables of the batch,
// builds libjpeg's canonical decode tables, packs the frame descriptors and the payloads into one pinned buffer and copies it
// with one asynchronous copy; k_jpeg.hip does the rest.
#include <algorithm>
#include <map>
#include <new>
#include <string.h>
#include <vector>

#include "ck_internal.h"
#include "ck_jpeg.h"
#include "ck_jpeg_tables.h"

namespace {

struct HuffSpec {
    bool present = false;
    uint8_t bits[17] = {};  // codes of each length 1..16
    uint8_t vals[256] = {};
    int nvals = 0;
};

struct Parsed {
    ck_jpeg_info_t info{};
    int ncomp = 0;
    int comp_id[3] = {}, comp_tq[3] = {};
    int scan_td[3] = {}, scan_ta[3] = {};
    bool qt_present[4] = {};
    uint16_t qt[4][64] = {};  // natural order
    HuffSpec dc[4], ac[4];
    int64_t scan_off = 0;     // first byte after the SOS header
};

// libjpeg's jpeg_make_d_derived_tbl checks: at most 256 symbols, the codes fit their lengths with the all-ones code of every
// length left unused, DC categories <= 15
bool huff_ok(const HuffSpec &t, bool dc) {
    int code = 0, p = 0;
    for (int l = 1; l <= 16; l++) {
        code += t.bits[l];
        p += t.bits[l];
        if (code >= (1 << l)) return false;
        code <<= 1;
    }
    if (p != t.nvals || p > 256) return false;
    if (dc)
        for (int i = 0; i < p; i++)
            if (t.vals[i] > 15) return false;
    return true;
}

// ITU-T T.81 Annex K.3: the tables a stream without DHT relies on, by class and slot 0 / 1
HuffSpec std_table(int cls, int slot) {
    const ck_jpeg_std_huff &k = kStdHuff[cls][slot];
    HuffSpec t;
    t.present = true;
    memcpy(t.bits + 1, k.bits, 16);
    memcpy(t.vals, k.vals, (size_t)k.n);
    t.nvals = k.n;
    return t;
}

int parse(const uint8_t *p, int64_t n, Parsed &P) {
    if (!p || n < 4 || p[0] != 0xFF || p[1] != 0xD8) return CK_EINVAL;
    int64_t i = 2;
    bool sof = false;
    int comp_h[3] = {}, comp_v[3] = {};
    int restart = 0;
    for (;;) {
        while (i < n && p[i] != 0xFF) i++; // bytes between segments are skipped, as libjpeg skips them
        while (i < n && p[i] == 0xFF) i++; // fill bytes
        if (i >= n) return CK_EINVAL;      // header truncated before SOS
        const int m = p[i++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue; // no segment
        if (m == 0xD8 || m == 0xD9) return CK_EINVAL;                      // SOI again / EOI before any scan
        if (i + 2 > n) return CK_EINVAL;
        const int seglen = (p[i] << 8) | p[i + 1];
        if (seglen < 2 || i + seglen > n) return CK_EINVAL;
        const uint8_t *s = p + i + 2;
        const int sl = seglen - 2;
        i += seglen;
        if (m == 0xC0 || m == 0xC1) { // baseline / extended sequential, Huffman
            if (sof || sl < 6) return CK_EINVAL;
            sof = true;
            const int prec = s[0], height = (s[1] << 8) | s[2], width = (s[3] << 8) | s[4], nf = s[5];
            if (prec == 12) return CK_EUNSUPPORTED;
            if (prec != 8) return CK_EINVAL;
            if (width == 0 || nf == 0) return CK_EINVAL;
            if (sl < 6 + 3 * nf) return CK_EINVAL;
            if (height == 0) return CK_EUNSUPPORTED; // the height follows in a DNL marker
            if (nf != 1 && nf != 3) return CK_EUNSUPPORTED;
            P.ncomp = nf;
            for (int c = 0; c < nf; c++) {
                P.comp_id[c] = s[6 + 3 * c];
                comp_h[c] = s[7 + 3 * c] >> 4;
                comp_v[c] = s[7 + 3 * c] & 15;
                P.comp_tq[c] = s[8 + 3 * c];
                if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4 || P.comp_tq[c] > 3) return CK_EINVAL;
                for (int e = 0; e < c; e++)
                    if (P.comp_id[e] == P.comp_id[c]) return CK_EINVAL;
            }
            if (comp_h[0] > 2 || comp_v[0] > 2) return CK_EUNSUPPORTED;
            for (int c = 1; c < nf; c++)
                if (comp_h[c] != 1 || comp_v[c] != 1) return CK_EUNSUPPORTED;
            P.info.width = width; P.info.height = height; P.info.n_components = nf;
            P.info.h_samp = comp_h[0]; P.info.v_samp = comp_v[0];
        } else if ((m >= 0xC2 && m <= 0xCF) && m != 0xC4) { // progressive, lossless, hierarchical, arithmetic (and DAC)
            return CK_EUNSUPPORTED;
        } else if (m == 0xC4) { // DHT
            int o = 0;
            while (o < sl) {
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3 || o + 17 > sl) return CK_EINVAL;
                HuffSpec t;
                t.present = true;
                int cnt = 0;
                for (int l = 1; l <= 16; l++) { t.bits[l] = s[o + l]; cnt += t.bits[l]; }
                if (cnt > 256 || o + 17 + cnt > sl) return CK_EINVAL;
                memcpy(t.vals, s + o + 17, (size_t)cnt);
                t.nvals = cnt;
                if (!huff_ok(t, tc == 0)) return CK_EINVAL;
                (tc ? P.ac : P.dc)[th] = t;
                o += 17 + cnt;
            }
            P.info.has_dht = 1;
        } else if (m == 0xDB) { // DQT
            int o = 0;
            while (o < sl) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq > 1 || tq > 3 || o + 1 + 64 * (pq + 1) > sl) return CK_EINVAL;
                for (int k = 0; k < 64; k++)
                    P.qt[tq][kNatural[k]] = pq ? (uint16_t)((s[o + 1 + 2 * k] << 8) | s[o + 2 + 2 * k]) : s[o + 1 + k];
                P.qt_present[tq] = true;
                o += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) { // DRI
            if (sl != 2) return CK_EINVAL;
            restart = (s[0] << 8) | s[1];
        } else if (m == 0xDA) { // SOS
            if (!sof || sl < 1) return CK_EINVAL;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl < 1 + 2 * ns + 3) return CK_EINVAL;
            int idx[4];
            for (int c = 0; c < ns; c++) {
                const int cs = s[1 + 2 * c], td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 3 || ta > 3) return CK_EINVAL;
                idx[c] = -1;
                for (int e = 0; e < P.ncomp; e++)
                    if (P.comp_id[e] == cs) idx[c] = e;
                if (idx[c] < 0) return CK_EINVAL;
                for (int e = 0; e < c; e++)
                    if (idx[e] == idx[c]) return CK_EINVAL;
                if (c < 3) { P.scan_td[c] = td; P.scan_ta[c] = ta; }
            }
            const int ss = s[1 + 2 * ns], se = s[2 + 2 * ns], ahal = s[3 + 2 * ns];
            if (ss != 0 || se != 63 || ahal != 0) return CK_EINVAL; // a sequential scan's spectral selection / approximation
            if (ns != P.ncomp) return CK_EUNSUPPORTED;               // non-interleaved scans (one scan per component, or Y missing)
            for (int c = 0; c < ns; c++)
                if (idx[c] != c) return CK_EINVAL;                   // scan components follow the frame's order
            for (int c = 0; c < P.ncomp; c++) {
                if (!P.qt_present[P.comp_tq[c]]) return CK_EINVAL;
                // a missing table 0 / 1 is the standard one (libjpeg-turbo: jpeg_std_huff_table); 2 / 3 must have been sent
                if (!P.dc[P.scan_td[c]].present && P.scan_td[c] > 1) return CK_EINVAL;
                if (!P.ac[P.scan_ta[c]].present && P.scan_ta[c] > 1) return CK_EINVAL;
            }
            P.info.restart_interval = restart;
            P.scan_off = i;
            return CK_OK;
        }
        // APPn, COM and every other segment: skipped
    }
}

// libjpeg's derived table (jdhuff.c: jpeg_make_d_derived_tbl) in the device layout
void derive(const HuffSpec &t, ck_jpeg_huff &o) {
    memset(&o, 0, sizeof o);
    int code = 0, p = 0;
    for (int l = 1; l <= 16; l++) {
        if (t.bits[l]) {
            o.valoff[l] = p - code;
            for (int k = 0; k < t.bits[l]; k++, p++, code++)
                if (l <= 9)
                    for (int x = 0; x < (1 << (9 - l)); x++) o.look[(code << (9 - l)) | x] = (uint16_t)((l << 8) | t.vals[p]);
            o.maxcode[l] = code - 1;
        } else {
            o.maxcode[l] = -1;
        }
        code <<= 1;
    }
    o.maxcode[17] = -1;
    memcpy(o.vals, t.vals, 256);
}

size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }

// The Huffman and quantisation tables of a batch, each distinct one once, in the device layout
struct Tables {
    std::vector<ck_jpeg_huff> tabs;
    std::vector<int32_t> qts;
    std::map<std::vector<uint8_t>, int> tab_ix, qt_ix;
    int huff(const HuffSpec &t) {
        std::vector<uint8_t> key(t.bits, t.bits + 17);
        key.insert(key.end(), t.vals, t.vals + t.nvals);
        auto it = tab_ix.find(key);
        if (it != tab_ix.end()) return it->second;
        tabs.emplace_back();
        derive(t, tabs.back());
        const int ix = (int)tabs.size() - 1;
        tab_ix.emplace(std::move(key), ix);
        return ix;
    }
    int quant(const uint16_t *q) {
        std::vector<uint8_t> key(reinterpret_cast<const uint8_t *>(q), reinterpret_cast<const uint8_t *>(q) + 128);
        auto it = qt_ix.find(key);
        if (it == qt_ix.end()) {
            it = qt_ix.emplace(std::move(key), (int)(qts.size() / 64)).first;
            for (int k = 0; k < 64; k++) qts.push_back(q[k]);
        }
        return it->second;
    }
    void finish() {
        if (tabs.empty()) tabs.emplace_back(); // (every frame bad: the kernels still get valid pointers)
        if (qts.empty()) qts.assign(64, 0);
    }
};

// the Y coefficient store of a frame: the largest MCU grid a sw x sh stream can have (2 x 2 sampling)
// (the colour form: and one Cb and one Cr block per MCU, most of them at 1 x 1 sampling: 256 bytes per MCU)
size_t coef_blocks(int sw, int sh, bool color = false) {
    return (size_t)((sw + 15) / 16) * 2 * (size_t)((sh + 15) / 16) * 2 + (color ? 2 * (size_t)((sw + 7) / 8) * (size_t)((sh + 7) / 8) : 0);
}
// the two chroma planes of a frame of the colour form, cw x ch each (none for a grey stream), as its region of d_planes
size_t plane_bytes(const ck_jpeg_desc &d, int sw, int sh) {
    if (d.status || d.bpm == 1) return 0;
    const size_t hs = d.hs, vs = d.nyb / d.hs;
    return al16(2 * ((sw + hs - 1) / hs) * ((sh + vs - 1) / vs));
}

// The descriptor of one frame of `size` bytes that parse() answered with rc, for sw x sh streams: everything but its three
// offsets (and plane_off).  d.status != 0: the frame is staged as zeros and has no payload.  color: the chroma's quantisation tables too.
void describe(const Parsed &p, int rc, int64_t size, int sw, int sh, Tables &T, ck_jpeg_desc &d, bool color) {
    memset(&d, 0, sizeof d);
    if (rc != CK_OK) { d.status = rc == CK_EUNSUPPORTED ? CK_JPEG_UNSUPPORTED : CK_JPEG_CORRUPT; return; }
    if (p.info.width != sw || p.info.height != sh) { d.status = CK_JPEG_GEOMETRY; return; }
    const int64_t raw_len = size - p.scan_off;
    if (raw_len > ((int64_t)1 << 28)) { d.status = CK_JPEG_UNSUPPORTED; return; } // bit positions are 32-bit
    const int H = p.ncomp == 1 ? 1 : p.info.h_samp, V = p.ncomp == 1 ? 1 : p.info.v_samp;
    d.mcux = (uint32_t)((sw + 8 * H - 1) / (8 * H));
    const uint32_t mcuy = (uint32_t)((sh + 8 * V - 1) / (8 * V));
    d.nmcu = d.mcux * mcuy;
    d.nyb = (uint32_t)(H * V);
    d.bpm = p.ncomp == 1 ? 1u : d.nyb + 2;
    d.hs = (uint32_t)H;
    d.yblk_stride = d.mcux * H;
    d.yblk_rows = mcuy * V;
    d.restart = p.info.restart_interval ? (uint32_t)p.info.restart_interval : d.nmcu;
    d.nint = (d.nmcu + d.restart - 1) / d.restart;
    d.raw_len = (uint32_t)raw_len;
    d.sub_cap = d.nint + (uint32_t)(((uint64_t)raw_len * 8 + CK_JPEG_SUB_BITS - 1) / CK_JPEG_SUB_BITS) + 1;
    for (int c = 0; c < p.ncomp; c++) {
        const HuffSpec &dc = p.dc[p.scan_td[c]].present ? p.dc[p.scan_td[c]] : std_table(0, p.scan_td[c]);
        const HuffSpec &ac = p.ac[p.scan_ta[c]].present ? p.ac[p.scan_ta[c]] : std_table(1, p.scan_ta[c]);
        d.dc[c] = (uint16_t)T.huff(dc);
        d.ac[c] = (uint16_t)T.huff(ac);
    }
    d.qt = (uint32_t)T.quant(p.qt[p.comp_tq[0]]);
    if (color)
        for (int c = 1; c < p.ncomp; c++) d.qtc[c - 1] = (uint32_t)T.quant(p.qt[p.comp_tq[c]]);
}

// The staging buffer of a call: descriptors | tables | quant tables | payloads
struct Layout {
    size_t off_tab, off_qt, off_raw, head_bytes; // head_bytes: what precedes the payloads, unpadded
};
Layout layout(int n, const Tables &T) {
    Layout L;
    L.off_tab = al16(sizeof(ck_jpeg_desc) * (size_t)n);
    L.off_qt = L.off_tab + sizeof(ck_jpeg_huff) * T.tabs.size();
    L.head_bytes = L.off_qt + sizeof(int32_t) * T.qts.size();
    L.off_raw = al16(L.head_bytes);
    return L;
}
void stage_head(uint8_t *S, const Layout &L, const ck_jpeg_desc *D, int n, const Tables &T) {
    memcpy(S, D, sizeof(ck_jpeg_desc) * (size_t)n);
    memcpy(S + L.off_tab, T.tabs.data(), sizeof(ck_jpeg_huff) * T.tabs.size());
    memcpy(S + L.off_qt, T.qts.data(), sizeof(int32_t) * T.qts.size());
}
// one frame's scan and the zeros that pad its region to raw_len + 4 rounded up to 16
void stage_scan(uint8_t *dst, const uint8_t *scan, uint32_t raw_len) {
    memcpy(dst, scan, raw_len);
    memset(dst + raw_len, 0, al16((size_t)raw_len + 4) - raw_len);
}

// the status array of a workspace (fixed size) and the buffers whose size follows the streams
int ws_status(ck_jpeg_ws &J, int max_batch) {
    const int rc = J.h_status.reserve(sizeof(uint32_t) * (size_t)max_batch, true);
    return rc != CK_OK ? rc : J.d_status.reserve(sizeof(uint32_t) * (size_t)max_batch);
}
// (exact: a ring's workspace never grows, so it gets no headroom)
int ws_reserve(ck_jpeg_ws &J, size_t stage_bytes, size_t raw_bytes, size_t n_int, size_t n_sub, size_t coef_blocks_total, size_t plane_total,
               bool exact = false) {
    int rc = J.h_stage.reserve(stage_bytes, exact);
    if (rc == CK_OK) rc = J.d_in.reserve(stage_bytes, exact);
    if (rc == CK_OK) rc = J.d_compact.reserve(raw_bytes ? raw_bytes : 16, exact);
    if (rc == CK_OK) rc = J.d_int.reserve(sizeof(uint32_t) * (n_int ? n_int : 1), exact);
    if (rc == CK_OK) rc = J.d_sub.reserve(sizeof(ck_jpeg_sub) * (n_sub ? n_sub : 1), exact);
    if (rc == CK_OK) rc = J.d_coef.reserve(sizeof(int16_t) * 64 * coef_blocks_total, exact);
    if (rc == CK_OK && plane_total) rc = J.d_planes.reserve(plane_total, exact);
    return rc;
}

// decode + IDCT of the n frames whose staging (layout L, payloads at off_raw) is on its way to J.d_in on stream s, into dst turned by
// `orientation`, and the statuses on their way back to J.h_status: everything enqueued, nothing awaited
int enqueue_decode(const ck_jpeg_ws &J, hipStream_t s, int n, const Layout &L, size_t off_raw, const ck_dev_image &dst, int sw, int sh,
                   int orientation, bool color) {
    const int rc = ck_launch_jpeg(J, s, n, reinterpret_cast<const ck_jpeg_desc *>(J.d_in.p), reinterpret_cast<const ck_jpeg_huff *>(J.d_in + L.off_tab),
                                  reinterpret_cast<const int32_t *>(J.d_in + L.off_qt), J.d_in + off_raw, coef_blocks(sw, sh, color), dst, sw, sh, orientation,
                                  color);
    if (rc != CK_OK) return rc;
    CK_HIP(hipMemcpyAsync(J.h_status, J.d_status, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    return CK_OK;
}

// ck_upload_jpeg[_oriented | _color]: the handle's workspace, the handle's stream, the staged frames, and the two synchronisations
int jpeg_run(ck_handle *h, const ck_jpeg_frame_t *frames, int n, int orientation, uint32_t *jpeg_status, bool color = false) {
    CK_HIP(hipSetDevice(h->device));
    if (!ck_workspace(h->jpeg)) return CK_ENOMEM;
    ck_jpeg_ws &J = *h->jpeg;
    int rc = ws_status(J, h->cfg.max_batch); // (a no-op once the first call has allocated the pair)
    if (rc != CK_OK) return rc;
    if (n == 0) {
        ck_set_staged(h, 0);
        if (color) { h->n_jpeg_color = 0; h->jpeg_color_orientation = orientation; }
        return CK_OK;
    }
    h->n_jpeg_color = -1; // (the descriptors and planes are about to be rewritten)
    int sw, sh;
    ck_source_size(h->w, h->h, orientation, &sw, &sh);
    // ---- parse + deduplicate --------------------------------------------------------------------------------------------------
    std::vector<Parsed> P((size_t)n);
    std::vector<ck_jpeg_desc> D((size_t)n);
    Tables T;
    uint64_t raw_total = 0, int_total = 0, sub_total = 0, plane_total = 0;
    for (int f = 0; f < n; f++) {
        ck_jpeg_desc &d = D[f];
        describe(P[f], parse(frames[f].data, frames[f].size, P[f]), frames[f].size, sw, sh, T, d, color);
        if (d.status) continue;
        if (color) {
            d.plane_off = plane_total;
            plane_total += plane_bytes(d, sw, sh);
        }
        d.raw_off = raw_total;
        raw_total += al16((size_t)d.raw_len + 4);
        d.int_off = int_total;
        int_total += d.nint + 1;
        d.sub_off = sub_total;
        sub_total += d.sub_cap;
    }
    T.finish();
    // ---- stage: descriptors | tables | quant tables | payloads -----------------------------------------------------------------
    const Layout L = layout(n, T);
    const size_t total = L.off_raw + raw_total;
    rc = ws_reserve(J, total, raw_total, int_total, sub_total, coef_blocks(sw, sh, color) * (size_t)n, color ? plane_total + 16 : 0);
    if (rc != CK_OK) return rc;
    CK_HIP(hipStreamSynchronize(h->stream)); // (the staging buffer may still feed an earlier call's copy)
    uint8_t *S = J.h_stage;
    stage_head(S, L, D.data(), n, T);
    for (int f = 0; f < n; f++)
        if (!D[f].status) stage_scan(S + L.off_raw + D[f].raw_off, frames[f].data + P[f].scan_off, D[f].raw_len);
    CK_HIP(hipMemcpyAsync(J.d_in, S, total, hipMemcpyHostToDevice, h->stream));
    rc = enqueue_decode(J, h->stream, n, L, L.off_raw, ck_staged_image(h), sw, sh, orientation, color);
    if (rc != CK_OK) return rc;
    CK_HIP(hipStreamSynchronize(h->stream));
    if (jpeg_status) memcpy(jpeg_status, J.h_status, sizeof(uint32_t) * (size_t)n);
    ck_set_staged(h, n);
    if (color) { h->n_jpeg_color = n; h->jpeg_color_orientation = orientation; }
    return CK_OK;
}

int check_frames(const ck_handle *h, const ck_jpeg_frame_t *frames, int32_t n, int32_t orientation) {
    if (!h || !frames || n < 0 || !ck_orientation_ok(orientation)) return CK_EINVAL;
    if (n > h->cfg.max_batch) return CK_ECAPACITY;
    for (int i = 0; i < n; i++)
        if (!frames[i].data || frames[i].size < 4) return CK_EINVAL;
    return CK_OK;
}

} // namespace

extern "C" int ck_jpeg_info(const uint8_t *data, int64_t size, ck_jpeg_info_t *out) {
    if (!data || !out) return CK_EINVAL;
    Parsed p;
    const int rc = parse(data, size, p);
    if (rc == CK_OK) *out = p.info;
    return rc;
}

extern "C" int ck_upload_jpeg_oriented(ck_handle_t *h, const ck_jpeg_frame_t *frames, int32_t n, int32_t orientation, uint32_t *jpeg_status) {
    const int rc = check_frames(h, frames, n, orientation);
    if (rc != CK_OK) return rc;
    return jpeg_run(h, frames, n, orientation, jpeg_status);
}

extern "C" int ck_upload_jpeg_color(ck_handle_t *h, const ck_jpeg_frame_t *frames, int32_t n, int32_t orientation, uint32_t *jpeg_status) {
    const int rc = check_frames(h, frames, n, orientation);
    if (rc != CK_OK) return rc;
    return jpeg_run(h, frames, n, orientation, jpeg_status, true);
}

int ck_jpeg_color_source(ck_handle *h, ck_jpeg_color_src *out) {
    if (h->n_jpeg_color < 0) return CK_EINVAL;
    const ck_jpeg_ws &J = *h->jpeg;
    int sw, sh;
    ck_source_size(h->w, h->h, h->jpeg_color_orientation, &sw, &sh);
    *out = {ck_staged_image(h), reinterpret_cast<const ck_jpeg_desc *>(J.d_in.p), J.d_status, J.d_planes, h->n_jpeg_color, sw, sh, h->jpeg_color_orientation};
    return CK_OK;
}

extern "C" int ck_upload_jpeg(ck_handle_t *h, const ck_jpeg_frame_t *frames, int32_t n, uint32_t *jpeg_status) {
    return ck_upload_jpeg_oriented(h, frames, n, CK_ORIENT_NONE, jpeg_status);
}

extern "C" int ck_jpeg_luma_batch_oriented(ck_handle_t *h, const ck_jpeg_frame_t *frames, int32_t n, int32_t orientation, uint8_t *luma_out,
                                           uint32_t *jpeg_status) {
    if (!luma_out) return CK_EINVAL;
    int rc = check_frames(h, frames, n, orientation);
    if (rc != CK_OK) return rc;
    rc = jpeg_run(h, frames, n, orientation, jpeg_status);
    if (rc != CK_OK || n == 0) return rc;
    rc = ck_read_staged_luma(h, n, luma_out);
    if (rc != CK_OK) return rc;
    CK_HIP(hipStreamSynchronize(h->stream));
    return CK_OK;
}

extern "C" int ck_jpeg_luma_batch(ck_handle_t *h, const ck_jpeg_frame_t *frames, int32_t n, uint8_t *luma_out, uint32_t *jpeg_status) {
    return ck_jpeg_luma_batch_oriented(h, frames, n, CK_ORIENT_NONE, luma_out, jpeg_status);
}

// ---- the JPEG half of an ingest ring ------------------------------------------------------------------------------------------
// A slot's staging has a fixed layout, so that ck_ingest_write_jpeg can place a frame's scan before the slot's tables are known:
// head_cap bytes for descriptors | tables | quant tables (their worst case: six Huffman tables and one quantisation table per frame),
// then one region of frame_cap bytes per frame index.  Submit copies the head with one copy and the regions of frames [0, n), as far
// as the longest scan reaches, with one pitched copy.
struct ck_jpeg_slots {
    ck_handle *h;
    int nslots, orientation, sw, sh;
    bool color;
    int64_t max_frame_bytes;
    size_t frame_cap, head_cap, int_cap, sub_cap, plane_cap; // plane_cap: a frame's region of d_planes (1 x 1 sampling), 0 without colour
    struct Slot {
        ck_jpeg_ws J;
        std::vector<Parsed> P;
        std::vector<int> rc;
        std::vector<int64_t> size;
        std::vector<uint8_t> written;
        std::vector<ck_jpeg_desc> D;
    } slot[8];
};

void ck_jpeg_slots_free(ck_jpeg_slots *q) { delete q; }

int ck_jpeg_slots_create(ck_handle *h, int n_slots, int orientation, int64_t max_frame_bytes, bool color, ck_jpeg_slots **out) {
    ck_jpeg_slots *q = new (std::nothrow) ck_jpeg_slots();
    if (!q) return CK_ENOMEM;
    q->h = h; q->nslots = n_slots; q->orientation = orientation; q->color = color;
    ck_source_size(h->w, h->h, orientation, &q->sw, &q->sh);
    q->plane_cap = color ? al16(2 * (size_t)q->sw * q->sh) : 0;
    q->max_frame_bytes = max_frame_bytes ? max_frame_bytes : (int64_t)q->sw * q->sh;
    const size_t nb = (size_t)h->cfg.max_batch;
    q->frame_cap = al16((size_t)q->max_frame_bytes + 4);
    // (the colour form: three quantisation tables per frame)
    q->head_cap = al16(al16(sizeof(ck_jpeg_desc) * nb) + sizeof(ck_jpeg_huff) * 6 * nb + sizeof(int32_t) * 64 * nb * (color ? 3 : 1));
    // a frame has at most one restart interval per MCU and at most one MCU per 8 x 8 pixels; its subsequences: ck_jpeg_desc::sub_cap
    const size_t nmcu_max = (size_t)((q->sw + 7) / 8) * (size_t)((q->sh + 7) / 8);
    q->int_cap = (nmcu_max + 1) * nb;
    q->sub_cap = (nmcu_max + ((size_t)q->max_frame_bytes * 8 + CK_JPEG_SUB_BITS - 1) / CK_JPEG_SUB_BITS + 1) * nb;
    int rc = CK_OK;
    try {
        for (int s = 0; s < n_slots; s++) {
            ck_jpeg_slots::Slot &S = q->slot[s];
            S.P.resize(nb); S.rc.assign(nb, CK_EINVAL); S.size.assign(nb, 0); S.written.assign(nb, 0); S.D.resize(nb);
        }
    } catch (const std::bad_alloc &) { rc = CK_ENOMEM; }
    for (int s = 0; s < n_slots && rc == CK_OK; s++) {
        ck_jpeg_ws &J = q->slot[s].J;
        rc = ws_status(J, h->cfg.max_batch);
        if (rc == CK_OK) rc = ws_reserve(J, q->head_cap + q->frame_cap * nb, q->frame_cap * nb, q->int_cap, q->sub_cap, coef_blocks(q->sw, q->sh, color) * nb,
                                            q->plane_cap * nb, true);
    }
    if (rc != CK_OK) { ck_jpeg_slots_free(q); return rc; }
    *out = q;
    return CK_OK;
}

int ck_jpeg_slots_write(ck_jpeg_slots *q, int slot, int index, const uint8_t *data, int64_t size) {
    if (size > q->max_frame_bytes) return CK_ECAPACITY;
    ck_jpeg_slots::Slot &S = q->slot[slot];
    Parsed &p = S.P[index];
    p = Parsed();
    const int rc = parse(data, size, p);
    S.rc[index] = rc;
    S.size[index] = size;
    // (a frame that describe() will refuse at submit has no payload; the same tests as there)
    if (rc == CK_OK && p.info.width == q->sw && p.info.height == q->sh && size - p.scan_off <= ((int64_t)1 << 28))
        stage_scan(S.J.h_stage + q->head_cap + q->frame_cap * (size_t)index, data + p.scan_off, (uint32_t)(size - p.scan_off));
    S.written[index] = 1;
    return CK_OK;
}

int ck_jpeg_slots_submit(ck_jpeg_slots *q, int slot, int n, hipStream_t s, const ck_dev_image &dst) {
    ck_jpeg_slots::Slot &S = q->slot[slot];
    for (int f = 0; f < n; f++)
        if (!S.written[f]) return CK_EINVAL;
    if (n == 0) return CK_OK;
    Tables T;
    uint64_t int_total = 0, sub_total = 0;
    size_t longest = 0;
    for (int f = 0; f < n; f++) {
        ck_jpeg_desc &d = S.D[f];
        describe(S.P[f], S.rc[f], S.size[f], q->sw, q->sh, T, d, q->color);
        if (d.status) continue;
        d.plane_off = q->plane_cap * (uint64_t)f;
        d.raw_off = q->frame_cap * (uint64_t)f; // its unstuffed copy lands at the same offset of d_compact
        d.int_off = int_total;
        int_total += d.nint + 1;
        d.sub_off = sub_total;
        sub_total += d.sub_cap;
        if (al16((size_t)d.raw_len + 4) > longest) longest = al16((size_t)d.raw_len + 4);
    }
    T.finish();
    const Layout L = layout(n, T);
    if (L.head_bytes > q->head_cap || int_total > q->int_cap || sub_total > q->sub_cap || longest > q->frame_cap) return CK_ECAPACITY; // (cannot happen: the caps are the worst case)
    const ck_jpeg_ws &J = S.J;
    stage_head(J.h_stage, L, S.D.data(), n, T);
    CK_HIP(hipMemcpyAsync(J.d_in, J.h_stage, L.head_bytes, hipMemcpyHostToDevice, s));
    if (longest)
        CK_HIP(hipMemcpy2DAsync(J.d_in + q->head_cap, q->frame_cap, J.h_stage + q->head_cap, q->frame_cap, longest, (size_t)n, hipMemcpyHostToDevice, s));
    const int rc = enqueue_decode(J, s, n, L, q->head_cap, dst, q->sw, q->sh, q->orientation, q->color);
    if (rc != CK_OK) return rc;
    std::fill(S.written.begin(), S.written.end(), (uint8_t)0);
    return CK_OK;
}

bool ck_jpeg_slots_color_source(const ck_jpeg_slots *q, int slot, const ck_dev_image &img, int n_frames, ck_jpeg_color_src *out) {
    if (!q->color) return false;
    const ck_jpeg_ws &J = q->slot[slot].J;
    *out = {img, reinterpret_cast<const ck_jpeg_desc *>(J.d_in.p), J.d_status, J.d_planes, n_frames, q->sw, q->sh, q->orientation};
    return true;
}

const uint32_t *ck_jpeg_slots_status(const ck_jpeg_slots *q, int slot) { return q->slot[slot].J.h_status; }
