// pw_resident.cpp — the query volumes kept on the device across the grid (pw_resident.h)
#include "pw_resident.h"

#include <algorithm>

#include "pw_common.h"

struct ResidentVolume {
    HostVolume hv;               // pac released once the bytes are on the device (and the volume file, if still being written, is done)
    mhip_volume* dv = NULL;
    size_t bytes = 0;
};
static std::vector<ResidentVolume*> g_resident;
static size_t g_resident_bytes = 0;
void resident_clear() {
    for (ResidentVolume* r : g_resident)
        if (r) { if (r->dv) mhip_volume_free(r->dv); delete r; }
    g_resident.clear();
    g_resident_bytes = 0;
}
mhip_volume* resident_get(mhip_ctx* ctx, const std::vector<std::string>& vn, int vid, const HostVolume** hv_out, HostVolume* own_host, bool* cached) {
    if (g_resident.size() < vn.size()) g_resident.resize(vn.size(), NULL);
    if (g_resident[(size_t)vid]) { *hv_out = &g_resident[(size_t)vid]->hv; *cached = true; return g_resident[(size_t)vid]->dv; }
    size_t budget;
    if (const char* e = getenv("MECAT_HIP_VOLCACHE_MB")) budget = (size_t)std::max(0L, atol(e)) << 20;
    else {
        size_t free_b = 0, total_b = 0;
        MCHK(mhip_ctx_mem_info(ctx, &free_b, &total_b));
        budget = total_b / 4;
    }
    HostVolume tmp;
    { TraceTimer tt("load_volume"); load_volume(vn[(size_t)vid], &tmp); }
    mhip_volume* dv = NULL;
    {
        TraceTimer tt("volume_upload");
        // (the packed bytes sit in huge pages the packer / reader has touched: locking them takes a few milliseconds and the copy then runs
        // at the link's rate instead of through the runtime's staging buffers)
        const bool locked = !tmp.pac.empty() && mhip_host_register(tmp.pac.data(), tmp.pac.size()) == 0;
        MCHK(mhip_volume_upload(ctx, tmp.pac.data(), tmp.offs.data(), tmp.num_reads, tmp.num_bases, tmp.start_read_id, &dv));
        if (locked) mhip_host_unregister(tmp.pac.data());
    }
    const size_t bytes = tmp.pac.size() + sizeof(mhip_offset_t) * tmp.offs.size();
    if (g_resident_bytes + bytes <= budget) {
        ResidentVolume* r = new ResidentVolume();
        r->hv = std::move(tmp);
        // the bytes live on the device now — unless the file of the volume that stayed in memory is still being written from these very
        // bytes (one-volume runs: nothing waits for that write; the host copy then goes with the cache)
        if (!volume_dump_in_flight()) { std::vector<uint8_t, NoInitAlloc<uint8_t>> none; r->hv.pac.swap(none); }
        r->dv = dv;
        r->bytes = bytes;
        g_resident[(size_t)vid] = r;
        g_resident_bytes += bytes;
        *hv_out = &r->hv;
        *cached = true;
        return dv;
    }
    *own_host = std::move(tmp);
    *hv_out = own_host;
    *cached = false;
    return dv;
}
