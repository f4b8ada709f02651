// The one thread-local message behind every error code, and every getter of the C ABI that reads it.  See errors.h.
#include "errors.h"

#include "../../include/ace_sfno.h"

namespace ace {

static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
const char* last_error() { return g_err.c_str(); }

}  // namespace ace

extern "C" {
const char* ace_last_error(void) { return ace::last_error(); }
const char* ace_mask_last_error(void) { return ace::last_error(); }
const char* ace_couple_last_error(void) { return ace::last_error(); }
const char* ace_diag_last_error(void) { return ace::last_error(); }
const char* ace_physics_last_error(void) { return ace::last_error(); }
const char* ace_hpx_last_error(void) { return ace::last_error(); }
const char* ace_ll_last_error(void) { return ace::last_error(); }
const char* ace_ocean_phys_last_error(void) { return ace::last_error(); }
const char* ace_ocean_derive_last_error(void) { return ace::last_error(); }
const char* ace_ice_budget_last_error(void) { return ace::last_error(); }
const char* ace_pixel_mlp_last_error(void) { return ace::last_error(); }
const char* ace_disco_last_error(void) { return ace::last_error(); }
}
