// pw_resident.h — query volumes that stay on the device across the grid rows
#pragma once

#include <string>
#include <vector>

#include "mecat_hip.h"
#include "volume.h"

// Query volumes stay RESIDENT across the grid: row i visits volumes i .. V - 1, row i + 1 visits i + 1 .. V - 1 again, and loading a 535 MB
// volume file, page-locking it, uploading it and freeing it again cost ~0.09 s per cell — 16 of the 43 s of config 5's `-j 0` run (190
// cells).  A volume is uploaded once per process and kept (device: the packed bytes and read table; host: the read table the formatter
// needs) while the resident volumes stay inside a budget of a quarter of the device memory (MECAT_HIP_VOLCACHE_MB overrides; 0 turns
// the cache off); volumes beyond the budget are loaded per cell as before.
void resident_clear();
// volume `vid`, on the device: from the cache, or loaded + uploaded now (and kept when it fits the budget: *cached says so; a volume that
// is not kept is the caller's to free, host part in *own_host, device part in the return value)
mhip_volume* resident_get(mhip_ctx* ctx, const std::vector<std::string>& vn, int vid, const HostVolume** hv_out, HostVolume* own_host, bool* cached);
